// The n-gram model's arguments, the table's slot and its exact-key lookup, shared by the kernels that read an NgramLM on the
// device (ngram.hip: scores of finished hypotheses and the terms of candidate next tokens; beam.hip: the LM state of every
// prefix inside the fused beam search).
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

struct NgModel {           // the arguments of oe_ngram_score that describe the model
    const float2* unigrams;
    const uint4* table;
    const int* tok2word;
    unsigned long long mask;   // capacity - 1
    int n_words, max_probe, order, bos_word, eos_word, unk_word, V;
};

// word id of a token: <unk> for a token outside [0, V) and for one the map sends outside the vocabulary
__device__ __forceinline__ int ng_word(const NgModel& m, int tok) {
    int w = (tok >= 0 && tok < m.V) ? m.tok2word[tok] : m.unk_word;
    if (w < 0 || w >= m.n_words) w = m.unk_word;
    return w;
}

// Host: the checks every entry point makes on an oe_ngram_model (include/openeat_hip.h; fn: the entry point's name, for the
// messages; the struct's pointers and V are the caller's to check), then the model as the kernels take it.
static inline int ng_model_args(const char* fn, const oe_ngram_model* a, NgModel* m) {
    OE_REQUIRE(a->order >= 1 && a->order <= NG_MAXORDER, "%s: order must be 1..%d (got %d)", fn, NG_MAXORDER, a->order);
    OE_REQUIRE(a->capacity >= 2 && (a->capacity & (a->capacity - 1)) == 0, "%s: capacity must be a power of two >= 2 (got %ld)", fn,
               a->capacity);
    OE_REQUIRE(a->max_probe >= 0 && a->max_probe < a->capacity, "%s: bad max_probe %d", fn, a->max_probe);
    OE_REQUIRE(a->n_words > 0 && (long)a->n_words + a->capacity < 0x7fffffffL, "%s: n_words + capacity must stay below 2^31", fn);
    OE_REQUIRE(a->bos_word >= 0 && a->bos_word < a->n_words && a->eos_word >= 0 && a->eos_word < a->n_words && a->unk_word >= 0 &&
               a->unk_word < a->n_words, "%s: <s> / </s> / <unk> ids outside the vocabulary", fn);
    m->unigrams = (const float2*)a->unigrams; m->table = (const uint4*)a->table; m->tok2word = a->tok2word;
    m->mask = (unsigned long long)(a->capacity - 1);
    m->n_words = a->n_words; m->max_probe = a->max_probe; m->order = a->order;
    m->bos_word = a->bos_word; m->eos_word = a->eos_word; m->unk_word = a->unk_word; m->V = a->V;
    return 0;
}
