// The streaming TTL output's monostable (csrc/trigger_pulse.hpp, what syldet_trigger_arm / syldet_trigger_render run) on its own:
// createHighOutput sets, renderOutput writes i < high ? 1 : 0 and counts down by min(high, frames).  Built with
// -fsanitize=address,undefined by tests/test_trigger_host.py; every buffer is exactly as long as the frames asked for.
#include <cstdio>
#include <thread>
#include <vector>

#include "trigger_pulse.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static std::vector<float> render(std::atomic<int64_t> &high, int n)
{
    std::vector<float> out((size_t)n, -1.0f);
    sd::trigger_pulse_render(high, out.data(), n);
    return out;
}

static int ones(const std::vector<float> &v)
{
    int n = 0;
    for (float x : v) {
        CHECK(x == 0.0f || x == 1.0f);
        n += x == 1.0f;
    }
    return n;
}

int main()
{
    std::atomic<int64_t> high{0};
    // never armed: zeros, and the counter stays
    CHECK(ones(render(high, 32)) == 0 && high.load() == 0);
    // 44 samples over buffers of 32: 32 ones, then 12 ones and 20 zeros, then zeros
    sd::trigger_pulse_arm(high, 44);
    std::vector<float> a = render(high, 32), b = render(high, 32), c = render(high, 32);
    CHECK(ones(a) == 32 && high.load() == 0);
    CHECK(ones(b) == 12 && b[11] == 1.0f && b[12] == 0.0f);
    CHECK(ones(c) == 0);
    // set, not added: an arm inside a pulse leaves its own width, not the sum
    sd::trigger_pulse_arm(high, 44);
    (void)render(high, 32);
    CHECK(high.load() == 12);
    sd::trigger_pulse_arm(high, 44);
    CHECK(high.load() == 44);
    CHECK(ones(render(high, 32)) == 32 && ones(render(high, 32)) == 12 && high.load() == 0);
    // a pulse shorter than a buffer, a pulse of exactly one buffer, frames beyond the pulse, an empty render
    sd::trigger_pulse_arm(high, 1);
    a = render(high, 8);
    CHECK(ones(a) == 1 && a[0] == 1.0f && high.load() == 0);
    sd::trigger_pulse_arm(high, 8);
    CHECK(ones(render(high, 8)) == 8 && ones(render(high, 8)) == 0);
    sd::trigger_pulse_arm(high, 5);
    CHECK(render(high, 0).empty() && high.load() == 5);
    CHECK(ones(render(high, 3)) == 3 && high.load() == 2 && ones(render(high, 1)) == 1 && ones(render(high, 4096)) == 1);
    // an arm of 0 ends a pulse
    sd::trigger_pulse_arm(high, 100);
    sd::trigger_pulse_arm(high, 0);
    CHECK(ones(render(high, 32)) == 0);
    // a renderer beside an armer: every frame is 0 or 1, the counter never goes below 0 and ends inside [0, 44]
    std::thread armer([&] { for (int i = 0; i < 20000; i++) sd::trigger_pulse_arm(high, 44); });
    for (int i = 0; i < 20000; i++) {
        (void)ones(render(high, 32));
        CHECK(high.load() >= 0 && high.load() <= 44);
    }
    armer.join();
    std::printf(failures ? "FAILED\n" : "ok\n");
    return failures ? 1 : 0;
}
