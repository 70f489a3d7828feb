// Long-form CTC segmentation (Kuerzinger et al. 2020): the best path of a whole recording through the trellis of its
// concatenated transcript, with free audio before and after it.  The semantics every layer refers to are in
// include/openeat_hip.h (oe_ctc_segment); the tie rule is oe_ctc_align's.
//
// oe_ctc_align keeps a T x (2L+1) float table of log-probabilities and runs one wave per utterance: 255 labels at most.
// A recording is T ~ 45 000 frames x S ~ 14 000 states, 6e8 cells: no float per cell fits, and one wave cannot hold a
// frame.  Two launches:
//   launch 1  seg_rows_kernel: one wave per frame, (c_t, lp[t,0]) with c_t = max + log sum exp(x - max) of the row, so that
//             lp[t,v] = logits[t,v] - c_t wherever it is needed later.  8 bytes per frame; no T x S table.
//   launch 2  seg_kernel<NS, CH>: ONE WORKGROUP PER RECORDING, up to 1024 threads, NS consecutive states per thread
//             (NS = 4 / 8 / 16 for S <= 4096 / 8192 / 16384; the block is ceil(S / NS) threads rounded up to whole waves).
//     recursion  v[t,s] = lp[t,ext[s]] + max(stay, step, skip) in float32.  NS is even, so a thread's even slots are
//                blanks and its odd slots labels, and the ONLY value it needs from its neighbour is the neighbour's last
//                state (the step into its blank and the skip into its first label): one DPP shift inside a wave
//                (wave_shr1, as ctc.hip), one float per wave through LDS across waves (double-buffered by frame parity:
//                one workgroup barrier per frame).  A thread needs logits[t, y[l]] for its NS / 2 labels; blank and c_t
//                come from launch 1.  Two routes, chosen from V and Lmax alone: where the workgroup can load a row coalesced
//                with at most SEG_RPT elements per thread and two rows fit SEG_ROWS_LDS, the rows of a chunk of two
//                frames are staged in LDS (loaded to registers a chunk ahead, stored when the chunk in hand is done) and the
//                labels are gathered from there; else every thread gathers from the rows themselves CH frames ahead.  The
//                scattered gather costs the vector L1 a tag lookup per lane and label, 7000 a frame at the bench shape against
//                the row's 133 lines: staging took the call from 136.8 to 85.2 ms there.  Each frame leaves 2 bits per state (0 stay /
//                1 step / 2 skip) in the workspace: a thread's NS moves are one 1 / 2 / 4-byte word, a frame's words one
//                coalesced row of `rowb` bytes; the moves of state s sit at bit 2 s of the row whatever NS is.
//     back-trace one dependent chain of Tb steps on wave 0, in tiles of 64 frames.  The state moves down by at most 2 per
//                frame, so the bytes a tile can need are known from the state at the tile's top: while a tile is walked
//                (its window in LDS), the window of the NEXT tile - 72 bytes of each of its 64 rows, cut from the state
//                the current tile began with - is already in flight in registers.
//     outputs    frames / path_logp in tiles of 64; first / last frame of every label in a table in the workspace; then
//                one thread per label sums its span (fixed order), and wave 0 adds the path's log-probabilities in
//                float64 in frame order.
// Nothing waits for another workgroup: no flags, no grid sync, no atomics - a recording's frames advance on its own
// workgroup's barriers only.  No allocation, no host read, no host-side state: capturable.
// Bound: a latency chain of Tb barrier-separated steps (DPP + LDS edge + 3-way max over NS states), then a chain of Tb
// LDS-resident back-trace steps; the logits' rows are read once per frame from HBM / L2.  Tried and dropped (measured
// slower, 95.6 against 85.2 ms): the maxima as v_max with the moves as two compare flags per state and the two free
// states in a rarely taken branch - fewer vector instructions per frame, but the step is not bound by their count.
#include <stdlib.h>
#include <type_traits>
#include "oe_common.h"
#include "../../include/openeat_hip.h"

#define SEG_NEG (-1.0e30f)          // finite "log 0" (see ctc.hip): SEG_NEG + lp stays SEG_NEG in fp32
#define SEG_MAX_T (1 << 20)
#define SEG_MAX_L 8191
#define SEG_WIN 72                  // bytes of a frame's back-pointer row a back-trace tile may need (see seg_window)
#define SEG_WIN_DW (SEG_WIN / 4)
#define SEG_RPT 8                   // staged rows: elements of a row per thread
#define SEG_ROWS_CH 2               // ... and frames per chunk
#define SEG_ROWS_LDS (48 * 1024)    // ... and their LDS (beside 9 KiB of static LDS, inside the 64 KiB a launch may ask for)

// lane i <- lane i-1, lane 0 <- SEG_NEG (row shift right by one across the whole wave)
__device__ __forceinline__ float seg_shr1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, SEG_NEG), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}

// ---------------------------------------------------------------- launch 1 ----
__global__ __launch_bounds__(256) void seg_rows_kernel(const float* __restrict__ logits, long ldv, long rows, int T, int V,
                                                        const int* __restrict__ hlens, float2* __restrict__ stat, size_t per_rec) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int b = (int)(row / T), t = (int)(row % T);
    if (t >= hlens[b]) return;
    const float* p = logits + row * ldv;
    float m = -INFINITY;
    for (int i = lane; i < V; i += 64) m = fmaxf(m, p[i]);
    m = wave_max(m);
    float s = 0.f;
    for (int i = lane; i < V; i += 64) s += expf(p[i] - m);
    s = wave_sum(s);
    const float c = m + logf(s);
    float2* st = reinterpret_cast<float2*>(reinterpret_cast<char*>(stat) + (size_t)b * per_rec);
    if (lane == 0) st[t] = make_float2(c, p[0] - c);
}

// ---------------------------------------------------------------- launch 2 ----
struct SegParams {
    const float* logits; long ldv; int T, V;
    const int* hlens; const int* targets; int Lmax; const int* tlens;
    int free_start, free_end;
    int* frames; float* path_logp; int* tok_start; int* tok_end; float* tok_logp; double* score;
    char* ws; size_t per_rec, rowb;      // per recording: [T * rowb back-pointers][T float2 stat][T float path lp][2 Lmax int spans]
};

// The window of back-pointer bytes that covers every state a walk can reach within 127 frames below a frame whose state
// is s: states [s - 254, s] are bits [2 s - 508, 2 s + 1] of a row, bytes [(s - 254) >> 2, s >> 2]; from the dword-aligned
// byte0 that is at most 18 dwords (SEG_WIN).
__device__ __forceinline__ int seg_window(int s) { return (max(s - 254, 0) >> 2) & ~3; }

// a lane's frame t of a back-trace window: the dwords from byte0 up to the one that holds state smax, zero elsewhere
__device__ __forceinline__ void seg_fetch(const char* bp, size_t rowb, int Tb, int t, int byte0, int smax, unsigned (&r)[SEG_WIN_DW]) {
    const unsigned* row = reinterpret_cast<const unsigned*>(bp + (size_t)max(t, 0) * rowb + (size_t)byte0);
    const int nd = (t >= 1 && t < Tb) ? ((smax >> 2) - byte0) / 4 + 1 : 0;      // inside the row: (smax >> 2) < rowb
#pragma unroll
    for (int d = 0; d < SEG_WIN_DW; ++d) r[d] = d < nd ? row[d] : 0u;
}

template <int NS, int CH, bool ROWS>
__global__ __launch_bounds__(1024) void seg_kernel(const SegParams p) {
    static_assert(NS % 4 == 0 && NS <= 16, "a thread's moves fill whole bytes of one word");
    typedef typename std::conditional<NS == 4, unsigned char, typename std::conditional<NS == 8, unsigned short, unsigned>::type>::type BPT;
    constexpr int NL = NS / 2;
    __shared__ float edge[2][16];                    // last state of every wave, by frame parity
    __shared__ float fin[2];                         // v[Tb-1, 2L], v[Tb-1, 2L-1]
    __shared__ unsigned win[2][64][SEG_WIN_DW];      // back-trace: window of the tile in hand / the next one
    extern __shared__ __attribute__((aligned(16))) float rows_sh[];      // ROWS: the logits' rows of the chunk in hand, CH x V

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int T = p.T, V = p.V, Lmax = p.Lmax;
    const long ldv = p.ldv;
    const int Tb = max(min(p.hlens[b], T), 0);
    const int L = max(min(p.tlens[b], Lmax), 0);
    const int S = 2 * L + 1;
    const bool fs = p.free_start != 0, fe = p.free_end != 0;
    const int* tg = p.targets + (long)b * Lmax;
    const float* lg = p.logits + (long)b * T * ldv;
    char* wsb = p.ws + (size_t)b * p.per_rec;
    const size_t rowb = p.rowb;
    char* bp = wsb;
    const float2* stat = reinterpret_cast<const float2*>(wsb + (size_t)T * rowb);
    float* plp = reinterpret_cast<float*>(wsb + (size_t)T * rowb + (size_t)T * 8);
    int* span = reinterpret_cast<int*>(wsb + (size_t)T * rowb + (size_t)T * 12);      // [0, Lmax) first frames, [Lmax, 2 Lmax) last
    int* fr = p.frames + (long)b * T;
    float* pl = p.path_logp ? p.path_logp + (long)b * T : nullptr;

    for (int l = tid; l < 2 * Lmax; l += blockDim.x) span[l] = -1;
    if (tid < 2) fin[tid] = SEG_NEG;
    __syncthreads();

    bool feasible = false;
    if (Tb > 0) {
        // ---- recursion
        const int s0 = tid * NS;
        const int endj = (fe && !(fs && L == 0)) ? (S - 1) - s0 : -1;       // slot of state 2L under free_end (even; else out of range)
        const bool zero0 = fs && tid == 0;                                   // state 0 under free_start
        int col[NL];
        unsigned skipm = 0;
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int s = s0 + 2 * k + 1, l = s >> 1;
            int c = 0;
            if (s < S) {
                c = min(max(tg[l], 0), V - 1);                               // a label outside [0, V) must not become a wild read
                if (l >= 1 && c != min(max(tg[l - 1], 0), V - 1)) skipm |= 1u << k;
            }
            col[k] = c;
        }
        float a[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) a[j] = SEG_NEG;
        {
            const float2 q0 = stat[0];
            if (tid == 0) {
                a[0] = fs ? 0.f : q0.y;
                if (S > 1) a[1] = lg[col[0]] - q0.x;
            }
        }
        float cur[CH][NL], nxt[ROWS ? 1 : CH][NL], nr[ROWS ? CH : 1][SEG_RPT];
        float2 curq[CH], nxtq[CH];
        const int nt = blockDim.x;
        // ROWS: the rows of frames tbase .. tbase + CH - 1, every thread SEG_RPT strided elements of each (coalesced)
        auto load_rows = [&](int tbase) {
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const float* rp = lg + (long)min(tbase + i, Tb - 1) * ldv;  // clamped: always a row of this recording
#pragma unroll
                for (int k = 0; k < SEG_RPT; ++k) {
                    const int c = tid + k * nt;
                    nr[ROWS ? i : 0][k] = c < V ? rp[c] : 0.f;
                }
            }
        };
        auto store_rows = [&]() {
#pragma unroll
            for (int i = 0; i < CH; ++i)
#pragma unroll
                for (int k = 0; k < SEG_RPT; ++k) {
                    const int c = tid + k * nt;
                    if (c < V) rows_sh[i * V + c] = nr[ROWS ? i : 0][k];
                }
        };
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int tt = min(1 + i, Tb - 1);
            if (!ROWS) {
                const float* rp = lg + (long)tt * ldv;
#pragma unroll
                for (int k = 0; k < NL; ++k) cur[i][k] = rp[col[k]];
            }
            curq[i] = stat[tt];
        }
        if (ROWS) {
            load_rows(1);
            store_rows();
        }
        for (int c0 = 1; c0 < Tb; c0 += CH) {
            if (ROWS) {
                // The chunk's rows are in LDS: gather the labels' logits from there (one cache line per lane and label from the
                // logits themselves costs the vector L1 a tag lookup each: 7000 per frame against the row's 133 lines), then
                // put the next chunk's rows in flight.  They are stored after the chunk's last frame: every thread has passed a
                // frame's barrier by then, and its gathers were complete before it arrived there.
                __syncthreads();
#pragma unroll
                for (int i = 0; i < CH; ++i)
#pragma unroll
                    for (int k = 0; k < NL; ++k) cur[i][k] = rows_sh[i * V + col[k]];
                load_rows(c0 + CH);
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int tt = min(c0 + CH + i, Tb - 1);                    // clamped: always a row of this recording
                if (!ROWS) {
                    const float* rp = lg + (long)tt * ldv;
#pragma unroll
                    for (int k = 0; k < NL; ++k) nxt[i][k] = rp[col[k]];
                }
                nxtq[i] = stat[tt];
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int t = c0 + i;
                if (t < Tb) {                                                // uniform over the workgroup
                    if (lane == 63) edge[t & 1][wave] = a[NS - 1];
                    __syncthreads();
                    float p1 = seg_shr1(a[NS - 1]);
                    if (lane == 0 && wave > 0) p1 = edge[t & 1][wave - 1];
                    const float cq = curq[i].x, lpb = curq[i].y;
                    float na[NS];
                    unsigned w = 0;
#pragma unroll
                    for (int j = 0; j < NS; ++j) {
                        const float n1 = (j >= 1) ? a[j >= 1 ? j - 1 : 0] : p1;
                        // a predecessor replaces the best only if strictly greater, in the order stay, step, skip
                        float best = a[j];
                        unsigned mv = 0;
                        if (n1 > best) { best = n1; mv = 1; }
                        if (j & 1) {
                            const float n2 = ((skipm >> (j >> 1)) & 1u) ? ((j >= 2) ? a[j >= 2 ? j - 2 : 0] : p1) : SEG_NEG;
                            if (n2 > best) { best = n2; mv = 2; }
                            na[j] = best + (cur[i][j >> 1] - cq);
                        } else {
                            na[j] = best + lpb;
                            if (j == endj) {                                 // free_end: staying in 2L is free, entering costs the blank
                                const float stepv = n1 + lpb;
                                mv = stepv > a[j] ? 1u : 0u;
                                na[j] = mv ? stepv : a[j];
                            }
                            if (j == 0 && zero0) { na[j] = 0.f; mv = 0; }
                        }
                        w |= mv << (2 * j);
                    }
#pragma unroll
                    for (int j = 0; j < NS; ++j) a[j] = na[j];
                    reinterpret_cast<BPT*>(bp + (size_t)t * rowb)[tid] = (BPT)w;
                }
            }
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                if (!ROWS) {
#pragma unroll
                    for (int k = 0; k < NL; ++k) {
                        cur[i][k] = nxt[i][k];
                        asm volatile("" : "+v"(cur[i][k]));
                    }
                }
                curq[i] = nxtq[i];
            }
            if (ROWS) store_rows();
        }
        // ---- end state: 2L unless 2L-1 is strictly greater
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            if (s0 + j == S - 1) fin[0] = a[j];
            if (s0 + j == S - 2) fin[1] = a[j];
        }
        __syncthreads();                                                     // also: every back-pointer row is written
        const float e0 = fin[0], e1 = fin[1];
        const float best = (e1 > e0) ? e1 : e0;
        feasible = best > 0.5f * SEG_NEG;
        if (feasible && wave == 0) {
            // ---- back-trace (wave 0)
            int s = (e1 > e0) ? S - 2 : S - 1;
            const int ttop = (Tb - 1) & ~63;
            unsigned r[SEG_WIN_DW];
            int byte0 = seg_window(s);
            seg_fetch(bp, rowb, Tb, ttop + lane, byte0, s, r);
#pragma unroll
            for (int d = 0; d < SEG_WIN_DW; ++d) win[0][lane][d] = r[d];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            int above = -1, buf = 0;
            for (int t0 = ttop; t0 >= 0; t0 -= 64) {
                const int thi = min(Tb - 1, t0 + 63);
                const int nbyte0 = seg_window(s);
                if (t0 > 0) seg_fetch(bp, rowb, Tb, t0 - 64 + lane, nbyte0, s, r);                    // in flight under the walk
                const unsigned char* wb = reinterpret_cast<const unsigned char*>(&win[buf][0][0]);
                int myS = -1, myMv = 0;
                for (int t = thi; t >= t0; --t) {
                    const int mv = (t == 0) ? 0 : (wb[(t & 63) * SEG_WIN + ((s >> 2) - byte0)] >> ((s & 3) * 2)) & 3;
                    if (lane == (t & 63)) { myS = s; myMv = mv; }
                    s = max(s - mv, 0);
                }
                if (t0 > 0) {
#pragma unroll
                    for (int d = 0; d < SEG_WIN_DW; ++d) win[buf ^ 1][lane][d] = r[d];
                }
                const int t = t0 + lane;
                const int up = __shfl_down(myS, 1, 64);
                if (t <= thi) {
                    const bool lab = myS & 1;
                    const int c = lab ? min(max(tg[myS >> 1], 0), V - 1) : 0;
                    const bool fre = (fs && myS == 0) || (fe && t > 0 && myS == S - 1 && myMv == 0);
                    const float x = fre ? 0.f : lg[(long)t * ldv + c] - stat[t].x;
                    fr[t] = lab ? tg[myS >> 1] : 0;
                    plp[t] = x;
                    if (pl) pl[t] = x;
                    if (lab) {
                        if (myMv != 0 || t == 0) span[myS >> 1] = t;
                        if ((t == thi ? above : up) != myS) span[Lmax + (myS >> 1)] = t;
                    }
                }
                above = __builtin_amdgcn_readfirstlane(myS);
                byte0 = nbyte0;
                buf ^= 1;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    for (int t = (feasible ? Tb : 0) + tid; t < T; t += blockDim.x) {
        fr[t] = -1;
        if (pl) pl[t] = 0.f;
    }
    __syncthreads();                                                         // spans and path lp of wave 0 -> the workgroup
    // ---- spans: one thread per label, a fixed summation order
    for (int l = tid; l < Lmax; l += blockDim.x) {
        const int st = (feasible && l < L) ? span[l] : -1, en = (feasible && l < L) ? span[Lmax + l] : -1;
        if (p.tok_start) p.tok_start[(long)b * Lmax + l] = st;
        if (p.tok_end) p.tok_end[(long)b * Lmax + l] = en;
        if (p.tok_logp) {
            float acc = 0.f;
            if (st >= 0) {
                const int c = min(max(tg[l], 0), V - 1);
                for (int t = st; t <= en; ++t) acc += lg[(long)t * ldv + c] - stat[t].x;
            }
            p.tok_logp[(long)b * Lmax + l] = acc;
        }
    }
    // ---- score: float64, frame order
    if (wave == 0) {
        double acc = feasible ? 0.0 : (double)-INFINITY;
        if (feasible) {
            float x = lane < Tb ? plp[lane] : 0.f;
            for (int t0 = 0; t0 < Tb; t0 += 64) {
                const int tn = t0 + 64 + lane;
                const float xn = tn < Tb ? plp[tn] : 0.f;                    // the next tile, under this tile's chain of additions
#pragma unroll 16
                for (int k = 0; k < 64; ++k) acc += (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), k));
                x = xn;
            }
        }
        if (lane == 0) p.score[b] = acc;
    }
}

// ---------------------------------------------------------------- host -------
// states per thread, threads per recording, bytes of a frame's back-pointer row
static inline int seg_ns(int Sp) { return Sp <= 4096 ? 4 : Sp <= 8192 ? 8 : 16; }
static inline int seg_threads(int Sp) { const int ns = seg_ns(Sp); return ((Sp + ns - 1) / ns + 63) & ~63; }
static inline size_t seg_rowb(int Sp) { return (size_t)seg_threads(Sp) * seg_ns(Sp) / 4; }
static inline size_t seg_per_rec(int T, int Lmax) {
    const int Sp = 2 * Lmax + 1;
    return ((size_t)T * (seg_rowb(Sp) + 12) + (size_t)8 * Lmax + 63) & ~(size_t)63;
}

extern "C" size_t oe_ctc_segment_workspace_bytes(int B, int T, int V, int Lmax) {
    (void)V;
    if (B <= 0 || T <= 0 || T > SEG_MAX_T || Lmax < 0 || Lmax > SEG_MAX_L) return 0;
    return (size_t)B * seg_per_rec(T, Lmax);
}

extern "C" int oe_ctc_segment(const oe_ctc_segment_args* args, void* stream) {
    OE_REQUIRE(args, "oe_ctc_segment: null args");
    const oe_ctc_segment_args& a = *args;
    OE_REQUIRE(a.logits && a.hlens && a.tlens && a.frames && a.score && a.workspace, "oe_ctc_segment: null pointer");
    OE_REQUIRE(a.targets || a.Lmax == 0, "oe_ctc_segment: null targets");
    OE_REQUIRE(a.B > 0 && a.T > 0 && a.T <= SEG_MAX_T && a.V > 1 && a.Lmax >= 0 && a.ldv >= a.V,
               "oe_ctc_segment: bad shape B=%d T=%d V=%d Lmax=%d ldv=%ld (1 <= T <= 2^20)", a.B, a.T, a.V, a.Lmax, a.ldv);
    OE_REQUIRE(a.Lmax <= SEG_MAX_L, "oe_ctc_segment: target length %d exceeds the %d-label limit of a workgroup", a.Lmax, SEG_MAX_L);
    OE_REQUIRE((((uintptr_t)a.workspace) & 15) == 0, "oe_ctc_segment: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int Sp = 2 * a.Lmax + 1;
    SegParams p;
    p.logits = a.logits; p.ldv = a.ldv; p.T = a.T; p.V = a.V;
    p.hlens = a.hlens; p.targets = a.targets; p.Lmax = a.Lmax; p.tlens = a.tlens;
    p.free_start = a.free_start; p.free_end = a.free_end;
    p.frames = a.frames; p.path_logp = a.path_logp; p.tok_start = a.tok_start; p.tok_end = a.tok_end; p.tok_logp = a.tok_logp;
    p.score = a.score;
    p.ws = reinterpret_cast<char*>(a.workspace); p.per_rec = seg_per_rec(a.T, a.Lmax); p.rowb = seg_rowb(Sp);
    const long rows = (long)a.B * a.T;
    float2* stat = reinterpret_cast<float2*>(p.ws + (size_t)a.T * p.rowb);
    hipLaunchKernelGGL(seg_rows_kernel, dim3(oe_cdiv(rows, 4)), dim3(256), 0, st, a.logits, a.ldv, rows, a.T, a.V, a.hlens, stat, p.per_rec);
    OE_LAUNCH_CHECK("ctc_segment_rows");
    const int nt = seg_threads(Sp);
    // The chunk's rows go through LDS where the workgroup can load them coalesced (SEG_RPT elements per thread) and two of them
    // fit; else every thread gathers its labels' logits from the rows themselves.  The route depends on V and Lmax only.
    const bool staged = (long)a.V <= (long)SEG_RPT * nt && (size_t)SEG_ROWS_CH * a.V * sizeof(float) <= SEG_ROWS_LDS;
    const size_t shm = staged ? (size_t)SEG_ROWS_CH * a.V * sizeof(float) : 0;
#define SEG(NS, CH) do { if (staged) hipLaunchKernelGGL((seg_kernel<NS, SEG_ROWS_CH, true>), dim3(a.B), dim3(nt), shm, st, p);  \
                         else hipLaunchKernelGGL((seg_kernel<NS, CH, false>), dim3(a.B), dim3(nt), 0, st, p); } while (0)
    switch (seg_ns(Sp)) {
        case 4: SEG(4, 8); break;
        case 8: SEG(8, 4); break;
        default: SEG(16, 2); break;
    }
#undef SEG
    OE_LAUNCH_CHECK("ctc_segment");
    return 0;
}
