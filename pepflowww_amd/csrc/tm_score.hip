// pf_tm_score_fwd -- TM-score with a fixed residue correspondence (the TMscore program's search, Zhang & Skolnick 2004) over a work
// list of pairs, in fp64.
//
// Launch 1 (tm_search_kernel): one LANE per (pair, seed).  A wave takes 64 consecutive seeds of one pair, four waves per 256-thread
// block, each wave on its own.  The wave compacts the pair's aligned points into its LDS slice (ballot + prefix popcount), then
// every lane runs its seed's whole search alone: Kabsch on the seed, score + cut, up to 20 refinements.  The lane's cut sets are
// bit masks in registers (NW 32-bit words, a template parameter, so every index is static); all lanes walk the points in the same
// order, so each LDS read is a broadcast.  Nothing is reduced across lanes until the end, where the wave picks its best candidate
// with an order-independent maximum on (score, -candidate index) and writes it, with the fp64 transform, to its scratch slot.
// Launch 2 (tm_finish_kernel): one wave per pair reduces the pair's slots the same way and writes the outputs.
#include <climits>

#include "common.h"
#include "../../include/pepflow_hip.h"
#include "superpose_dev.h"
#include "eval_dev.h"

namespace {

constexpr int TM_CAND = 21;                 // superpositions scored per seed: the seed and up to 20 refinements

struct TmSlot {                             // best candidate of one wave (64 seeds of one pair)
    double score;                           // -1: none
    long long cand;                         // seed index * TM_CAND + iteration; LLONG_MAX: none
    double rt[12];                          // rot (row-major), trans
};

// seed lengths: n, n/2, ... while above min(4, n), then min(4, n) (at most five halvings)
__host__ __device__ inline int tm_seed_lengths(int n, int Ls[6]) {
    const int lmin = n < 4 ? n : 4;
    int c = 0;
    for (int m = 0; m < 5; ++m) {
        const int v = n >> m;
        if (v <= lmin) {
            Ls[c++] = lmin;
            return c;
        }
        Ls[c++] = v;
    }
    Ls[c++] = lmin;
    return c;
}

__host__ __device__ inline int tm_seed_count(int n) {
    int Ls[6];
    const int c = tm_seed_lengths(n, Ls);
    int s = 0;
    for (int i = 0; i < c; ++i) s += n - Ls[i] + 1;
    return s;
}

// 64-seed chunks per pair for point sets of up to N points
inline int tm_chunks(int N) {
    int most = 0;
    for (int n = 3; n <= N; ++n) {
        const int c = tm_seed_count(n);
        most = c > most ? c : most;
    }
    return most > 0 ? (most + 63) / 64 : 1;
}

__device__ __forceinline__ void tm_point(const float* pts, int k, double xv[3], double yv[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        xv[c] = pts[6 * k + c];
        yv[c] = pts[6 * k + 3 + c];
    }
}

// proper Kabsch superposition of the points in S (centroids first, then the centred cross terms): y ~ R x + t
template <int NW>
__device__ void tm_kabsch(const float* pts, int n, const uint32_t (&S)[NW], double R[3][3], double t[3]) {
    double cnt = 0.0, sx[3] = {0.0, 0.0, 0.0}, sy[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (32 * w >= n) break;
        for (int b = 0; b < 32 && 32 * w + b < n; ++b) {
            if (!((S[w] >> b) & 1u)) continue;
            double xv[3], yv[3];
            tm_point(pts, 32 * w + b, xv, yv);
            cnt += 1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) { sx[c] += xv[c]; sy[c] += yv[c]; }
        }
    }
    double mx[3], my[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { mx[c] = sx[c] / cnt; my[c] = sy[c] / cnt; }
    double C[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (32 * w >= n) break;
        for (int b = 0; b < 32 && 32 * w + b < n; ++b) {
            if (!((S[w] >> b) & 1u)) continue;
            double xv[3], yv[3];
            tm_point(pts, 32 * w + b, xv, yv);
#pragma unroll
            for (int c = 0; c < 3; ++c) { xv[c] -= mx[c]; yv[c] -= my[c]; }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) C[r][c] += xv[r] * yv[c];
        }
    }
    double lam;
    kabsch_rotation(C, false, R, lam);
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = my[r] - (R[r][0] * mx[0] + R[r][1] * mx[1] + R[r][2] * mx[2]);
}

__device__ __forceinline__ double tm_d2(const float* pts, int k, const double R[3][3], const double t[3]) {
    double xv[3], yv[3];
    tm_point(pts, k, xv, yv);
    double d2 = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double e = R[r][0] * xv[0] + R[r][1] * xv[1] + R[r][2] * xv[2] + t[r] - yv[r];
        d2 += e * e;
    }
    return d2;
}

// sum over the aligned points of d0^2 / (d0^2 + d^2) at (R, t), and the cut: S = {k : d_k < d}, d raised by 0.5 until S has 3
// points (when n > 3).  The raised d is d + 0.5 m for the least such m, found from the third-smallest distance.
template <int NW>
__device__ double tm_score_cut(const float* pts, int n, const double R[3][3], const double t[3], double d0sq, double d,
                               uint32_t (&S)[NW]) {
    double sc = 0.0;
    int cnt = 0;
    const double dd = d * d;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        S[w] = 0u;
        if (32 * w >= n) continue;
        for (int b = 0; b < 32 && 32 * w + b < n; ++b) {
            const double d2 = tm_d2(pts, 32 * w + b, R, t);
            sc += d0sq / (d0sq + d2);
            const bool in = d2 < dd;
            S[w] |= (uint32_t)in << b;
            cnt += in;
        }
    }
    if (cnt < 3 && n > 3) {                                         // rare: fewer than 3 points inside d
        double m0 = __builtin_inf(), m1 = m0, m2 = m0;                // the three smallest d^2
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (32 * w >= n) break;
            for (int b = 0; b < 32 && 32 * w + b < n; ++b) {
                double v = tm_d2(pts, 32 * w + b, R, t);
                if (v < m0) { const double u = m0; m0 = v; v = u; }
                if (v < m1) { const double u = m1; m1 = v; v = u; }
                if (v < m2) m2 = v;
            }
        }
        if (!(m2 <= 1e300)) return sc;                              // non-finite input: leave the cut short
        double m = floor((sqrt(m2) - d) * 2.0) - 1.0;
        if (!(m > 0.0)) m = 0.0;
        double dm = d + 0.5 * m;
        for (int g = 0; g < 64 && !(m2 < dm * dm); ++g) {            // one or two steps; bounded for coordinates near FLT_MAX
            m += fmax(1.0, m * 0x1p-50);
            dm = d + 0.5 * m;
        }
        const double dd2 = dm * dm;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            S[w] = 0u;
            if (32 * w >= n) continue;
            for (int b = 0; b < 32 && 32 * w + b < n; ++b) S[w] |= (uint32_t)(tm_d2(pts, 32 * w + b, R, t) < dd2) << b;
        }
    }
    return sc;
}

struct TmPair {
    const float* X; const float* Y; const unsigned char* MX; const unsigned char* MY;
    bool valid;
};

__device__ __forceinline__ TmPair tm_pair(const pf_tm_score_args& a, int p) {
    const int i = a.pairs[2 * p], j = a.pairs[2 * p + 1];
    TmPair q;
    q.valid = i >= 0 && i < a.Bx && j >= 0 && j < a.By;
    q.X = a.x + (size_t)(q.valid ? i : 0) * a.N * 3;
    q.Y = a.y + (size_t)(q.valid ? j : 0) * a.N * 3;
    q.MX = a.mx + (size_t)(q.valid ? i : 0) * a.N;
    q.MY = a.my + (size_t)(q.valid ? j : 0) * a.N;
    return q;
}

__device__ __forceinline__ double tm_d0(int lnorm) {
    const double d0 = 1.24 * cbrt((double)lnorm - 15.0) - 1.8;
    return d0 > 0.5 ? d0 : 0.5;
}

template <int NW>
__global__ __launch_bounds__(256) void tm_search_kernel(pf_tm_score_args a, int nchunk, TmSlot* work) {
    extern __shared__ float tm_lds[];                               // per wave: N points x (x, y)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * 4 + wv;
    if (w >= (long long)a.P * nchunk) return;                       // whole waves only: no block barrier below
    const int p = (int)(w / nchunk), chunk = (int)(w % nchunk);
    const TmPair q = tm_pair(a, p);
    const int N = a.N;
    float* pts = tm_lds + (size_t)wv * N * 6;

    // compact the aligned points (mx & my, index order) into LDS; Lnorm = |my|
    int n = 0, lnorm = 0;
    if (q.valid)
        for (int base = 0; base < N; base += 64) {
            const int k = base + lane;
            const bool ym = k < N && q.MY[k];
            const bool both = ym && q.MX[k];
            const unsigned long long bal = __ballot(both);
            lnorm += __popcll(__ballot(ym));
            if (both) {
                const int pos = n + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    pts[6 * pos + c] = q.X[(size_t)k * 3 + c];
                    pts[6 * pos + 3 + c] = q.Y[(size_t)k * 3 + c];
                }
            }
            n += __popcll(bal);
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // this lane's seed: index sd of the pair's seed list (lengths in order, starts in order)
    const int sd = chunk * 64 + lane;
    int Ls = 0, s0 = 0;
    if (n >= 3) {
        int L[6];
        const int nl = tm_seed_lengths(n, L);
        int r = sd;
        for (int u = 0; u < nl; ++u) {
            const int c = n - L[u] + 1;
            if (r < c) { Ls = L[u]; s0 = r; break; }
            r -= c;
        }
    }

    double best = -1.0;
    long long bestc = LLONG_MAX;
    double bR[3][3], bt[3];
    if (Ls > 0) {
        const double d0 = tm_d0(lnorm), d0sq = d0 * d0;
        const double d0s = d0 < 4.5 ? 4.5 : (d0 > 8.0 ? 8.0 : d0);
        const double inv_l = 1.0 / (double)lnorm;
        uint32_t S[NW];
#pragma unroll
        for (int u = 0; u < NW; ++u) {                              // bits s0 .. s0 + Ls - 1
            const int lo = min(max(s0 - 32 * u, 0), 32), hi = min(max(s0 + Ls - 32 * u, 0), 32);
            const uint32_t below_hi = hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u);
            const uint32_t below_lo = lo >= 32 ? 0xffffffffu : ((1u << lo) - 1u);
            S[u] = below_hi & ~below_lo;
        }
        for (int it = 0; it < TM_CAND; ++it) {
            double R[3][3], t[3];
            tm_kabsch(pts, n, S, R, t);
            uint32_t Sn[NW];
            const double sc = tm_score_cut(pts, n, R, t, d0sq, it == 0 ? d0s - 1.0 : d0s + 1.0, Sn) * inv_l;
            if (sc > best) {
                best = sc;
                bestc = (long long)sd * TM_CAND + it;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    bt[r] = t[r];
#pragma unroll
                    for (int c = 0; c < 3; ++c) bR[r][c] = R[r][c];
                }
            }
            if (it == TM_CAND - 1) break;
            bool same = it > 0;
            int cnt = 0;
#pragma unroll
            for (int u = 0; u < NW; ++u) {
                same = same && Sn[u] == S[u];
                cnt += __popc(Sn[u]);
                S[u] = Sn[u];
            }
            if (same || cnt < 3) break;
        }
    }

    double wb = best;
    long long wc = bestc;
    wave_best(wb, wc);
    TmSlot* slot = work + (size_t)p * nchunk + chunk;
    if (lane == 0) {
        slot->score = wb;
        slot->cand = wc;
    }
    if (wc != LLONG_MAX && bestc == wc) {                           // the one lane that holds the winner
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            slot->rt[9 + r] = bt[r];
#pragma unroll
            for (int c = 0; c < 3; ++c) slot->rt[3 * r + c] = bR[r][c];
        }
    }
}

__global__ __launch_bounds__(256) void tm_finish_kernel(pf_tm_score_args a, int nchunk, const TmSlot* work) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.P) return;
    const TmPair q = tm_pair(a, p);
    const int N = a.N;
    int n = 0, lnorm = 0;
    if (q.valid)
        for (int base = 0; base < N; base += 64) {
            const int k = base + lane;
            const bool ym = k < N && q.MY[k];
            n += __popcll(__ballot(ym && q.MX[k]));
            lnorm += __popcll(__ballot(ym));
        }
    double s = -1.0;
    long long c = LLONG_MAX;
    for (int u = lane; u < nchunk; u += 64) {
        const TmSlot* sl = work + (size_t)p * nchunk + u;
        if (cand_better(sl->score, sl->cand, s, c)) { s = sl->score; c = sl->cand; }
    }
    wave_best(s, c);
    const bool ok = n >= 3 && c != LLONG_MAX;
    double R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}}, t[3];
    const float qnan = __int_as_float(0x7fc00000);
    if (ok) {
        const TmSlot* sl = work + (size_t)p * nchunk + (int)(c / TM_CAND / 64);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            t[r] = sl->rt[9 + r];
#pragma unroll
            for (int k = 0; k < 3; ++k) R[r][k] = sl->rt[3 * r + k];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) t[r] = qnan;
    }
    if (lane == 0) {
        a.tm[p] = ok ? (float)s : qnan;
        a.count[p] = n;
        a.lnorm[p] = lnorm;
        if (a.rot) {
#pragma unroll
            for (int k = 0; k < 9; ++k) a.rot[(size_t)p * 9 + k] = (float)R[k / 3][k % 3];
#pragma unroll
            for (int k = 0; k < 3; ++k) a.trans[(size_t)p * 3 + k] = (float)t[k];
        }
    }
    if (a.aligned)
        for (int k = lane; k < N; k += 64) {
            const double xv[3] = {q.X[(size_t)k * 3], q.X[(size_t)k * 3 + 1], q.X[(size_t)k * 3 + 2]};
#pragma unroll
            for (int r = 0; r < 3; ++r)
                a.aligned[((size_t)p * N + k) * 3 + r] =
                    ok ? (float)(R[r][0] * xv[0] + R[r][1] * xv[1] + R[r][2] * xv[2] + t[r]) : qnan;
        }
}

template <int NW>
void tm_launch_search(const pf_tm_score_args& a, int nchunk, unsigned blocks, hipStream_t stream) {
    hipLaunchKernelGGL(tm_search_kernel<NW>, dim3(blocks), dim3(256), (size_t)4 * a.N * 6 * sizeof(float), stream, a, nchunk,
                       (TmSlot*)a.work);
}

}  // namespace

static_assert(sizeof(TmSlot) == PF_TM_SLOT_BYTES, "slot layout");

extern "C" int pf_tm_score_work_slots(int N) {
    if (N < 1 || N > PF_TM_MAX_N) return -1;
    return tm_chunks(N);
}

extern "C" int pf_tm_score_fwd(const pf_tm_score_args* a, pf_stream_t stream) {
    if (!a || !a->x || !a->y || !a->mx || !a->my || !a->pairs || !a->tm || !a->count || !a->lnorm || a->Bx <= 0 || a->By <= 0 ||
        a->N <= 0 || a->P < 0 || (!a->rot != !a->trans) || (a->P > 0 && !a->work))
        return PF_E_BADARG;
    if (a->N > PF_TM_MAX_N) return PF_E_TOOLARGE;
    if (a->P == 0) return 0;
    const int nchunk = tm_chunks(a->N);
    const long long waves = (long long)a->P * nchunk;
    if ((waves + 3) / 4 > 0x7fffffffLL) return PF_E_TOOLARGE;
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    const hipStream_t s = (hipStream_t)stream;
    const int nw = (a->N + 31) / 32;
    if (nw <= 1) tm_launch_search<1>(*a, nchunk, blocks, s);
    else if (nw <= 2) tm_launch_search<2>(*a, nchunk, blocks, s);
    else if (nw <= 4) tm_launch_search<4>(*a, nchunk, blocks, s);
    else if (nw <= 8) tm_launch_search<8>(*a, nchunk, blocks, s);
    else tm_launch_search<16>(*a, nchunk, blocks, s);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(tm_finish_kernel, dim3((unsigned)((a->P + 3) / 4)), dim3(256), 0, s, *a, nchunk, (const TmSlot*)a->work);
    PF_CHECK_LAUNCH();
    return 0;
}
