// The n-gram table's slot and its exact-key lookup, shared by the kernels that read an NgramLM on the device
// (ngram.hip: scores of finished hypotheses; beam_lm.hip: the LM state of every prefix inside the beam search).
// Layout and key chaining: include/openeat_hip.h (oe_ngram_score) and openeat_amd/models/ngram_lm.py.
#pragma once
#include "oe_common.h"

#define NG_MAXORDER 5
#define NG_EMPTY 0xFFFFFFFFFFFFFFFFull

struct NgSlot {            // one 16-byte slot of the table
    unsigned long long key;
    float logp, backoff;
};

__device__ __forceinline__ unsigned long long ng_mix(unsigned long long x) {      // murmur3's 64-bit finaliser
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// slot of `key`, or -1; at most max_probe + 1 slots are read, every index is < cap
__device__ __forceinline__ long ng_find(const uint4* __restrict__ table, unsigned long long mask, int max_probe,
                                        unsigned long long key, float& logp, float& backoff) {
    unsigned long long slot = ng_mix(key) & mask;
    for (int d = 0; d <= max_probe; ++d) {
        const uint4 v = table[slot];
        const unsigned long long k = ((unsigned long long)v.y << 32) | v.x;
        if (k == key) { logp = __uint_as_float(v.z); backoff = __uint_as_float(v.w); return (long)slot; }
        if (k == NG_EMPTY) return -1;
        slot = (slot + 1) & mask;
    }
    return -1;
}
