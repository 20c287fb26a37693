// plx_philox.h -- the library's counter-based generator, shared by the kernels that draw noise on the device.
//
// Philox-4x32-10 (Salmon et al., SC'11): four 32-bit counter words, two key words, ten rounds.  Every draw is a pure
// function of (counter, key), so the noise of a realisation depends only on its key, never on how frames are batched
// or sharded over GPUs.  Key of a draw: k0 = lo32(seed ^ key), k1 = hi32(seed) ^ hi32(key * 0x9E3779B97F4A7C15).
// The fourth counter word separates the streams of one key:
//   0, 1  ASE of ampliflat, X / Y polarisation (plx_misc.hip, counter = (sample lo, sample hi, column, pol))
//   2     transmitter laser phase noise   (plx_phase.hip, counter = (sample lo, sample hi, channel, 2))
//   3     local-oscillator phase noise    (plx_phase.hip, counter = (sample lo, sample hi, channel, 3))
//   4     transmitted data, PLX_PHILOX_TX_DATA (plx_tx.hip, counter = (word group lo, word group hi, channel, 4): the four
//         words are 32 symbols of the four bit streams, no uniforms are formed)
// Uniforms from one call: u1 = ((r0 << 21) ^ (r1 >> 11) + 0.5) / 2^53, u2 = the same of (r2, r3); Box-Muller gives
// sqrt(-2 ln u1) * (cos 2 pi u2, sin 2 pi u2).
#pragma once
#include "plx_common.h"

namespace {
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                           uint32_t *out)
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
} // namespace
