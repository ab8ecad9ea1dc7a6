// The plain read of tools/ubench/read_bw.hip (grid-stride, 8 non-temporal 16-byte loads in flight a lane, 2048 workgroups) as a
// function a Python tool can time on a buffer of its own, launch by launch, beside the code under test (tools/levels_timing.py).
// Diagnostic, not part of the product.
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC -o tools/ubench/libplain_read.so tools/ubench/plain_read.hip
#include <hip/hip_runtime.h>
#include <cstddef>
typedef float floatx4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) plain_read_kernel(const floatx4 *__restrict__ p, size_t n, float *sink)
{
    constexpr int U = 8;
    floatx4 acc = {0, 0, 0, 0};
    const size_t stride = (size_t)gridDim.x * 256 * U;
    for (size_t i = (size_t)blockIdx.x * 256 * U + threadIdx.x; i < n; i += stride) {
        floatx4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = i + 256 * u < n ? __builtin_nontemporal_load(p + i + 256 * u) : floatx4{0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < U; u++) acc += v[u];
    }
    if (acc[0] + acc[1] + acc[2] + acc[3] == 12345.678f) sink[0] = acc[0];
}

// reads the first bytes / 16 16-byte elements of p (16-byte aligned); sink: 4 bytes of device memory
extern "C" int plain_read(const void *p, size_t bytes, float *sink, void *stream)
{
    hipLaunchKernelGGL(plain_read_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const floatx4 *)p, bytes / 16, sink);
    return (int)hipGetLastError();
}
