// vap_philox.h — the counter-based generator of the calls that draw numbers on the device (vap_search_sample,
// vap_velocity_conditioning): a draw is a function of (counter, key) alone, so a result does not depend on the launch shape.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vap {

struct uint4x {
    uint32_t x, y, z, w;
};

// Philox4x32-10 (Salmon et al., SC'11): counter c, key k
__device__ __forceinline__ uint4x philox4x32_10(uint4x c, uint32_t k0, uint32_t k1)
{
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = uint4x{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += W0;
        k1 += W1;
    }
    return c;
}

}  // namespace vap
