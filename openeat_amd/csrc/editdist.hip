// Batched edit distance on the device, one wavefront per (reference, hypothesis) pair: the counts (cor, sub, del, ins)
// behind the reference's error-rate table (tools/compute-wer.py, Calculator.calculate) and, on request, the alignment
// itself.  Semantics (the tie order included) in include/openeat_hip.h; the yardstick is tests/edit_distance_ref.py.
//
// Formulation: anti-diagonal wavefront.  Cell (i, j) of the (n+1) x (m+1) table lies on diagonal d = i + j and needs
// (i-1, j) and (i, j-1) from diagonal d-1 and (i-1, j-1) from d-2, so all cells of a diagonal are independent.  Lanes
// are laid across the reference: lane l owns rows i = l K + 1 .. l K + K (K = 1, 2, 4, 8 or 16 by Nmax) and keeps the
// last two diagonals of its rows in registers.  A step is then one full-wave DPP shift per diagonal kept (the row above
// a lane's first row belongs to lane l-1; row 0 enters lane 0 through the shift's `old` operand) and K cell updates;
// there are n + m steps.  The row sweep (n steps, the insertion chain as a wave prefix-min of t[k] - k) was the other
// candidate: it needs two dependent wave scans per row - the minimum, then a segmented copy that hands the carried
// counts along a run of insertions - which cost more than the n extra steps of the plain wavefront at these lengths
// (six dependent cross-lane steps per scan against one shift), and it has to recover the tie order after the fact.
// Here the tie order is literally the header's: del, then ins, then diagonal, replaced only if strictly smaller.
//
// What a cell carries: D << 16 | dl, its distance and the number of deletions on its chosen path.  The other counts
// follow from where the cell is: a path to (i, j) has cor + sub + del = i and cor + sub + ins = j, so
// ins = j - i + del, sub = D - del - ins, cor = i - sub - del.  The counts-only call therefore carries one integer
// forward and touches no workspace.  D <= 2046 and dl <= 1024 leave both halves far from overflow.
//
// The hypothesis is staged in LDS once; a lane's K cells read K consecutive tokens that slide by one per step, so they
// live in K registers fed by one LDS read a step, issued a step ahead.  Rows beyond n and columns beyond m compute
// garbage that nothing valid depends on (a cell only looks up and left); only their memory accesses are guarded.
//
// Aligned call: every cell also leaves its move (0 del / 1 ins / 2 diagonal) as 2 bits; a row belongs to one lane, which
// gathers 16 consecutive cells into a word and stores it to bp[(i-1) * W + (j-1) / 16], W = ceil(Mmax / 16).  The words
// are in LDS while Nmax * W * 4 bytes <= ED_LDS_BP = 48 KiB (three waves a CU next to the token stage), else in the
// workspace, P * Nmax * W words (the route depends on Nmax and Mmax only).  After a barrier the wave walks back from
// (n, m): one dependent load per row visited (a run of insertions stays inside the word in hand), lane 0 writes
// ref_to_hyp.  Bound: latency - n + m dependent steps, then at most n + m / 16 dependent loads.
#include "oe_common.h"
#include "../../include/openeat_hip.h"

#define ED_MAXLEN 1023
#define ED_LDS_BP (48 * 1024)

// lane l takes lane l-1's v; lane 0 takes `first`
__device__ __forceinline__ int ed_shr1(int v, int first) { return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false); }

// BP: 0 counts only, 1 back-pointers in LDS, 2 in the workspace
template <int K, int BP>
__global__ __launch_bounds__(64) void edit_distance_kernel(const int* __restrict__ ref, long ref_ld, const int* __restrict__ ref_lens,
                                                           int group, const int* __restrict__ hyp, long hyp_ld,
                                                           const int* __restrict__ hyp_lens, int Nmax, int Mmax,
                                                           int* __restrict__ counts, int* __restrict__ ref_to_hyp,
                                                           unsigned* __restrict__ bp_ws) {
    extern __shared__ int ed_sh[];                               // max(Mmax, 1) hypothesis tokens, then the LDS back-pointer words
    const int p = blockIdx.x, lane = threadIdx.x;
    const int m_raw = hyp_lens[p];
    int* al = BP ? ref_to_hyp + (long)p * Nmax : nullptr;
    if (m_raw < 0) {                                             // the slot does not exist (wave-uniform)
        if (lane < 4) counts[4 * (long)p + lane] = -1;
        if (BP) for (int i = lane; i < Nmax; i += 64) al[i] = -1;
        return;
    }
    const int u = p / group;
    const int n = min(max(ref_lens[u], 0), Nmax), m = min(m_raw, Mmax);
    const int* r = ref + (long)u * ref_ld;
    const int* h = hyp + (long)p * hyp_ld;
    const int hsN = max(Mmax, 1);
    int* hs = ed_sh;
    const int W = (Mmax + 15) >> 4;
    unsigned* bp = BP == 1 ? reinterpret_cast<unsigned*>(ed_sh + hsN) : BP == 2 ? bp_ws + (size_t)p * Nmax * W : nullptr;
    for (int j = lane; j < m; j += 64) hs[j] = h[j];
    __syncthreads();

    int res = m << 16;                                           // n == 0: m insertions
    if (n > 0) {
        const int i0 = lane * K;                                 // rows i0 + 1 .. i0 + K
        int rt[K], p1[K], p2[K], ht[K];
        unsigned word[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = i0 + 1 + k;
            rt[k] = i <= n ? r[i - 1] : 0;
            p1[k] = p2[k] = 0;
            ht[k] = 0;
            word[k] = 0u;
        }
        int hnext = hs[min(max(1 - i0 - 2, 0), hsN - 1)];
        const int steps = n + m;
        for (int d = 1; d <= steps; ++d) {
#pragma unroll
            for (int k = K - 1; k > 0; --k) ht[k] = ht[k - 1];
            ht[0] = hnext;                                       // token j - 1 of cell k = 0, j = d - i0 - 1
            hnext = hs[min(max(d - i0 - 1, 0), hsN - 1)];
            // the row above this lane's first: (i0, j) on diagonal d-1 and (i0, j-1) on d-2; row 0 is D[0][j] = j, no deletions
            const int a1 = ed_shr1(p1[K - 1], (d - 1) * 0x10000), a2 = ed_shr1(p2[K - 1], (d - 2) * 0x10000);
            int cur[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = i0 + 1 + k, j = d - i;
                const int up1 = k ? p1[k ? k - 1 : 0] : a1, up2 = k ? p2[k ? k - 1 : 0] : a2;
                // deletion, insertion, diagonal, in this order; a later one replaces the best only if strictly smaller
                int best = up1 + 0x10001;
                unsigned mv = 0u;
                const int ins = p1[k] + 0x10000;
                if ((ins >> 16) < (best >> 16)) { best = ins; mv = 1u; }
                const int dg = up2 + (rt[k] != ht[k] ? 0x10000 : 0);
                if ((dg >> 16) < (best >> 16)) { best = dg; mv = 2u; }
                cur[k] = j == 0 ? ((i << 16) | i) : best;        // D[i][0] = i, all deletions
                if (BP) {
                    const int c = (j - 1) & 15;
                    if (c == 0) word[k] = 0u;
                    word[k] |= mv << (2 * c);
                    if (i <= n && j >= 1 && j <= m && (c == 15 || j == m)) bp[(size_t)(i - 1) * W + ((j - 1) >> 4)] = word[k];
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) { p2[k] = p1[k]; p1[k] = cur[k]; }
        }
        // (n, m) was the one valid cell of the last diagonal
        int mine = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) if (i0 + 1 + k == n) mine = p1[k];
        res = __builtin_amdgcn_readlane(mine, __builtin_amdgcn_readfirstlane((n - 1) / K));
    }
    const int D = res >> 16, dl = res & 0xffff;
    const int ins = m - n + dl, sub = D - dl - ins, cor = n - sub - dl;
    if (lane < 4) counts[4 * (long)p + lane] = lane == 0 ? cor : lane == 1 ? sub : lane == 2 ? dl : ins;

    if (BP) {
        __syncthreads();                                         // every lane's words are visible to the walk
        int i = n, j = m, row = -1, col = -1;
        unsigned w = 0u;
        while (i > 0 && j > 0) {                                 // wave-uniform: all lanes walk, lane 0 writes
            const int wc = (j - 1) >> 4;
            if (i != row || wc != col) { w = bp[(size_t)(i - 1) * W + wc]; row = i; col = wc; }
            const unsigned mv = (w >> (2 * ((j - 1) & 15))) & 3u;
            if (mv == 0u) { if (lane == 0) al[i - 1] = -1; --i; }
            else if (mv == 1u) --j;
            else { if (lane == 0) al[i - 1] = j - 1; --i; --j; }
        }
        for (int t = lane; t < i; t += 64) al[t] = -1;           // column 0 reached: the rest are deletions
        for (int t = n + lane; t < Nmax; t += 64) al[t] = -1;
    }
}

static inline int ed_words(int Mmax) { return (Mmax + 15) >> 4; }
static inline bool ed_in_lds(int Nmax, int Mmax) { return (size_t)Nmax * ed_words(Mmax) * 4 <= ED_LDS_BP; }

extern "C" size_t oe_edit_distance_workspace_bytes(int P, int Nmax, int Mmax) {
    if (P <= 0 || Nmax <= 0 || Mmax < 0 || Nmax > ED_MAXLEN || Mmax > ED_MAXLEN || ed_in_lds(Nmax, Mmax)) return 0;
    return (size_t)P * Nmax * ed_words(Mmax) * 4;
}

extern "C" int oe_edit_distance(const int* ref, long ref_ld, const int* ref_lens, int group, const int* hyp, long hyp_ld,
                                const int* hyp_lens, int P, int Nmax, int Mmax, int* counts, int* ref_to_hyp, void* workspace,
                                void* stream) {
    OE_REQUIRE(ref_lens && hyp_lens && counts, "oe_edit_distance: null pointer");
    OE_REQUIRE(P >= 0 && Nmax >= 0 && Mmax >= 0, "oe_edit_distance: bad shape P=%d Nmax=%d Mmax=%d", P, Nmax, Mmax);
    OE_REQUIRE(Nmax <= ED_MAXLEN && Mmax <= ED_MAXLEN, "oe_edit_distance: Nmax=%d / Mmax=%d exceed the %d-token limit", Nmax, Mmax,
               ED_MAXLEN);
    OE_REQUIRE(group >= 1, "oe_edit_distance: group must be >= 1 (got %d)", group);
    OE_REQUIRE(P % group == 0, "oe_edit_distance: P=%d is not a multiple of group=%d", P, group);
    OE_REQUIRE(ref_ld >= Nmax && hyp_ld >= Mmax, "oe_edit_distance: leading dimensions %ld / %ld below Nmax=%d / Mmax=%d", ref_ld,
               hyp_ld, Nmax, Mmax);
    OE_REQUIRE((ref || Nmax == 0) && (hyp || Mmax == 0), "oe_edit_distance: null ref / hyp");
    const bool align = ref_to_hyp != nullptr && Nmax > 0;
    const bool in_lds = ed_in_lds(Nmax, Mmax);
    OE_REQUIRE(!align || in_lds || workspace, "oe_edit_distance: null workspace (oe_edit_distance_workspace_bytes)");
    if (P == 0) return 0;
    const size_t shm = (size_t)(Mmax > 0 ? Mmax : 1) * 4 + (align && in_lds ? (size_t)Nmax * ed_words(Mmax) * 4 : 0);
    const int bpm = !align ? 0 : in_lds ? 1 : 2;
#define ED(K, BP) hipLaunchKernelGGL((edit_distance_kernel<K, BP>), dim3(P), dim3(64), shm, (hipStream_t)stream, ref, ref_ld, ref_lens, group, \
                                     hyp, hyp_ld, hyp_lens, Nmax, Mmax, counts, ref_to_hyp, reinterpret_cast<unsigned*>(workspace))
#define EDK(K) do { if (bpm == 0) ED(K, 0); else if (bpm == 1) ED(K, 1); else ED(K, 2); } while (0)
    if (Nmax <= 64) EDK(1); else if (Nmax <= 128) EDK(2); else if (Nmax <= 256) EDK(4); else if (Nmax <= 512) EDK(8); else EDK(16);
#undef EDK
#undef ED
    OE_LAUNCH_CHECK("edit_distance");
    return 0;
}
