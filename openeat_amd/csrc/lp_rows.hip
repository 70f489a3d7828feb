// The row pass of the CTC decoders that work on a few columns of the posteriors: launch 1 of oe_ctc_kws, oe_ctc_graph,
// oe_ctc_graph_logp (and its gradient), oe_ctc_graph_beam and oe_ctc_graph_nbest.  One kernel, one launcher (oe_lp_rows,
// declared in oe_common.h).
//
//   launch 1  lp_rows_kernel: one wave per frame (as seg_rows_kernel).  The row is read once, coalesced, with its log-sum-exp
//             c_t taken on the way (one pass: a running maximum and a rescaled sum per lane, merged across the wave), and the
//             blank and the U keyword columns are gathered from the row just read (L1 / L2 hits) and written as
//             lp = x - c_t into a compact row of U + 1 floats.  normalized: no pass over the row, the gather alone.
//             lse (the gradient of oe_ctc_graph_logp): c_t is kept too, a float per row.
//             Bound: the logits' bytes from HBM, once.
// Rows with t >= hlens[b] are not written.  No waves wait for each other, no LDS, no atomics: capturable.
#include "oe_common.h"

__global__ __launch_bounds__(256) void lp_rows_kernel(const float* __restrict__ logits, long ldv, long rows, int T, int V,
                                                       const int* __restrict__ hlens, const int* __restrict__ cols, int U,
                                                       int normalized, float* __restrict__ cw, float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = (int)(row / T), t = (int)(row % T);
    if (t >= hlens[b]) return;
    const float* p = logits + row * ldv;
    float c = 0.f;
    if (!normalized) {
        // one pass: per lane a running maximum m and the sum of exp(x - m), eight elements in flight
        float m = -INFINITY, s = 0.f;
        int i = lane;
        for (; i + 7 * 64 < V; i += 8 * 64) {
            float x[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = p[i + k * 64];
            float mx = x[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) mx = fmaxf(mx, x[k]);
            if (mx > m) { s *= expf(m - mx); m = mx; }
#pragma unroll
            for (int k = 0; k < 8; ++k) s += expf(x[k] - m);
        }
        for (; i < V; i += 64) {
            const float x = p[i];
            if (x > m) { s *= expf(m - x); m = x; }
            s += expf(x - m);
        }
        const float wm = wave_max(m);
        s = wave_sum(m == -INFINITY ? 0.f : s * expf(m - wm));
        c = wm + logf(s);
    }
    if (lse && lane == 0) lse[row] = c;
    float* out = cw + row * (long)(U + 1);
    for (int u = lane; u <= U; u += 64) {
        const int col = u == 0 ? 0 : min(max(cols[u - 1], 0), V - 1);       // a label outside [0, V) must not become a wild read
        out[u] = p[col] - c;
    }
}

// who: the entry that calls ("oe_ctc_kws", ...), for the messages.  cw: B * T rows of U + 1 floats; lse: B * T floats or null.
int oe_lp_rows(const char* who, const float* logits, long ldv, int B, int T, int V, const int* hlens, const int* cols, int U,
               int normalized, float* cw, float* lse, hipStream_t st) {
    const long rows = (long)B * T;
    OE_REQUIRE(rows <= 0x7fffffffL, "%s: B * T = %ld rows exceed the grid limit", who, rows);
    hipLaunchKernelGGL(lp_rows_kernel, dim3(oe_cdiv(rows, 4)), dim3(256), 0, st, logits, ldv, rows, T, V, hlens, cols, U, normalized, cw,
                       lse);
    char name[64];
    snprintf(name, sizeof(name), "%s_rows", who);
    OE_LAUNCH_CHECK(name);
    return 0;
}
