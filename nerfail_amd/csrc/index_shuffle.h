// The index shuffle of nerfail_index_shuffle / nerfail_train_batch (include/nerfail_hip.h, ABI 13): P(key, m), a bijection of
// [0, m) evaluated per element - no table, no sort. index_shuffle() below IS the definition (rounds, mixer, key schedule);
// tests/batch_ref.py restates it in numpy and the GPU tests compare bit for bit, so any change here changes every batch
// a (seed, step) pair draws.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nerfail {

constexpr int kShuffleRounds = 6;

// murmur3's 32-bit finaliser
__host__ __device__ inline uint32_t shuffle_mix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// Balanced Feistel network over 2 * half bits, the smallest even width whose range covers m - 1 (at least 2), with
// cycle-walking: the network is re-applied while the value lies outside [0, m). The walk starts inside [0, m) and the network
// is a permutation of [0, 4^half), so it returns to [0, m) after at most 4^half - m + 1 steps (in practice a handful:
// 4^half < 4 m). Round r: (L, R) -> (R, L ^ (mix32(R ^ k_r) & mask)), k_r = mix32(key_lo ^ mix32(key_hi + (r + 1) * 0x9E3779B9)).
// Requires 1 <= m <= 2^31 and i < m.
__host__ __device__ inline uint32_t index_shuffle(uint64_t key, uint32_t m, uint32_t i) {
    int half = 1;
    while (half < 16 && (((uint64_t)1 << (2 * half)) < (uint64_t)m)) ++half;
    const uint32_t mask = (1u << half) - 1u;
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    uint32_t k[kShuffleRounds];
    for (int r = 0; r < kShuffleRounds; ++r) k[r] = shuffle_mix32(lo ^ shuffle_mix32(hi + (uint32_t)(r + 1) * 0x9E3779B9u));
    uint32_t x = i;
    do {
        uint32_t L = x >> half, R = x & mask;
        for (int r = 0; r < kShuffleRounds; ++r) {
            const uint32_t t = L ^ (shuffle_mix32(R ^ k[r]) & mask);
            L = R;
            R = t;
        }
        x = (L << half) | R;
    } while (x >= m);
    return x;
}

}  // namespace nerfail
