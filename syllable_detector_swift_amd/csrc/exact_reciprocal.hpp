// exact_reciprocal.hpp -- where dividing by an output gain may be a multiplication (host side: fused_plan.cpp;
// tests/cpp/exact_reciprocal_test.cpp).  The reverse output map is (y - y0) / gain + x0 (NeuralNet.swift:137-142 / :175-180).
// For a gain that is a power of two, 1 / gain is a power of two as well, so x * (1 / gain) and x / gain round the same real number:
// the same float for every x, products that overflow or go subnormal included, as long as 1 / gain itself is a normal float.
#pragma once

#include <cmath>

namespace sd {

// 1 / g where that is exact and normal: g a normal power of two of either sign below 2^127; 0 otherwise.
inline float exact_reciprocal_f32(float g)
{
    int e = 0;
    if (!std::isnormal(g) || std::fabs(std::frexp(g, &e)) != 0.5f) return 0.0f;
    const float r = 1.0f / g;
    return std::isnormal(r) ? r : 0.0f;
}

}  // namespace sd
