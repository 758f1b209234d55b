// pf_tm_align_fwd -- TM-align (Zhang & Skolnick, Nucleic Acids Res. 33, 2302, 2005): sequence-independent structural alignment of
// CA traces over a work list of pairs, in fp64 from the fp32 inputs.  X (chain 1, the model: x[i] with mx[i], compacted in index
// order, Lx residues) is superposed onto Y (chain 2, the target, Ly residues); an alignment is y2x[j] (-1 unaligned).
//
// Conventions (tests/tmalign_oracle.py restates them in numpy; the pipeline is TMalign_main without options):
//   Chains    Lx < 3 or Ly < 3: NaN scores, no alignment.
//   Search    Lmin = min(Lx, Ly); d0 = (Lmin <= 19 ? 0.168 : 1.24 cbrt(Lmin - 15) - 1.8) + 0.8 (also D0_MIN); d0_search = clamp(d0,
//             4.5, 8); score_d8 = 1.5 Lmin^0.3 + 3.5; ddcc = 0.1 (Lmin <= 40) or 0.4; scores normalised by Lmin while searching.
//   Fits      proper Kabsch in fp64 (superpose_dev.h).  Degenerate fits: 0 points -> identity, t = 0; 1 point -> identity, t = y - x;
//             2 points -> the smallest rotation taking unit(x1 - x0) onto unit(y1 - y0) (identity if either is zero; a half turn
//             about unit(a x e_k), k the axis of the smallest |a_k|, first on ties, when 1 + cos <= 1e-12); >= 3 points of rank < 2
//             (s2 <= 1e-6 s1) -> identity; t = mean(y) - R mean(x) in every case.
//   SS        make_sec without smoothing (TM-align 2019+): for 2 <= i < L - 2 the six CA distances among i-2 .. i+2; H if all within
//             2.1 of (6.37, 5.18, 5.18, 5.45, 5.45, 5.45) for (d15, d14, d25, d13, d24, d35), else E if all within 1.42 of (13,
//             10.4, 10.4, 6.1, 6.1, 6.1), else T if d15 < 8, else C; the two residues at each end are C.
//   DP        NWDP_TM: rows i over X, columns j over Y, val[i][0] = val[0][j] = 0; d = val[i-1][j-1] + s(i,j); h = val[i-1][j]
//             (+ gap if (i-1,j) was diagonal), v = val[i][j-1] (+ gap if (i,j-1) was diagonal); diagonal if d >= h && d >= v, else
//             val = v >= h ? v : h.  Traceback from (Lx, Ly): diagonal = a pair; else j-1 if v >= h, else i-1 (the 2-bit code kept
//             in the fill).  s = 1 / (1 + d^2 / d02) under the current transform (DP_iter: d02 = d0^2), [ss_i == ss_j] (gap -1),
//             or 1 / (1 + d^2 / d01^2) + 0.5 [ss_i == ss_j] (gap -1), d01 = d0 + 1.5.
//   TM search TMscore8_search on the La aligned pairs: seeds of lengths La, La/2, ... floored at min(4, La), starts 0, step, 2 step,
//             ... and always La - L; fit, cut at d0_search - 1, then up to 20 refits at d0_search + 1 on the cut set (d2 < d^2, d
//             raised by 0.5 m for the least m giving 3 pairs when La > 3); a seed stops when its cut set repeats or has < 3 pairs.
//             Score = sum 1 / (1 + d^2 / d0^2) / Lnorm, only over d^2 <= score_d8^2 while searching (score_sum_method 8).  The
//             first strictly greater candidate in (seed, iteration) order wins.  La = 0: score 0, the transform is left as it is.
//   Quick     get_score_fast: fit all pairs, score (not normalised); refit on d^2 <= d0_search^2 (+ 0.5 m, the least m giving 3
//             pairs when n > 3; the program adds 0.5 m times, here t2 + 0.5 m in one step), score; refit on d^2 <= d0_search^2 + 1
//             (raised the same way) under the second fit, score; the largest of the three.  The second cut keeping every pair skips
//             the last two fits.
//   Pipeline  1 gapless threading (min_ali = max(Lmin / 2, 5); shifts -Ly + min_ali .. Lx - min_ali, the last of equal quick scores;
//             none in range: k = -Ly + min_ali); 2 the SS DP; 3 local superposition (fragments min(20, Lmin / 3) and min(100,
//             Lmin / 2), start jumps 45 / 35 / 25 / 15 for L > 250 / 200 / 150 / else, capped at L / 3; first strictly greater
//             quick score; skipped when none is > 0); 4 SS plus superposition (Kabsch on the best alignment so far); 5 fragment
//             gapless threading (the first longest run of consecutive CAs with d^2 < dcu^2, dcu = 4.25 * 1.1^k, the factor by
//             repeated multiplication, raised until the run reaches min(4, L / 3), at most 1000 times; the x run if it is shorter,
//             or equal with Lx <= Ly, else the y run; a run as long as min(Lx, Ly) keeps its entries int(0.1 L0) .. int(0.89 L0);
//             min_ali = max(int(min(Lrun, L_other) / 2.5), 3); the last of equal quick scores; no shift in range: the map stays).
//             Each stage: a detailed search (step 40) that sets the transform and competes for the best (strictly greater); then
//             DP_iter (gaps -0.6 and 0, 30 iterations) in stage 1, in 2 if TM > 0.2 TMmax, in 4 if TM > ddcc TMmax; (-0.6 and 0, 2)
//             in 3 and (0, 2) in 5 if TM > ddcc TMmax.  DP_iter: per gap, per iteration a DP under the current transform, a step-40
//             search that sets the transform, keep the map if strictly better, stop the gap after the first iteration once
//             |TM - TM_old| < 1e-6 (TM_old carries over between the gaps).
//   Final     a step-1 search (method 8) on the best alignment sets the transform; the pairs with sqrt(d^2) <= score_d8 are kept
//             (n_aligned; rmsd = their Kabsch RMSD); tm_x and tm are step-1 searches over all kept pairs with d0 = 0.5 (L <= 21) or
//             max(0.5, 1.24 cbrt(L - 15) - 1.8), d0_search = clamp(d0, 4.5, 8), normalised by Lx and Ly; rot / trans come from tm's.
//
// One wave per pair (a 64-thread block), every stage in one launch, LDS sized at launch by the bound on the compacted lengths
// (max_len, default N).  Lanes run independent candidates: a shift each in stages 1 and 5, a seed each in every TM search (cut sets
// are bit masks in the lane's own LDS column).  The DP is an anti-diagonal wavefront: lane l holds row r0 + 1 + l of a 64-row strip,
// takes val[i-1][*] from lane l - 1 by shuffle (from the previous strip's last row in LDS for lane 0) and writes its 2-bit cell codes
// into its own LDS row; lane 0 walks the traceback.  Fits and quick scores of single candidates run redundantly on every lane, so
// uniform values need no broadcast.  Arg-maxima are order-independent maxima over (score, +-index).  No atomics, no scratch.
#include <climits>

#include "common.h"
#include "../../include/pepflow_hip.h"
#include "superpose_dev.h"
#include "eval_dev.h"

namespace {

constexpr int TA_CAND = 21;                 // superpositions per seed: the seed and up to 20 refits
constexpr int TA_STEP = 40;
constexpr int TA_FRAG_RAISES = 1000;

__device__ __forceinline__ void ta_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Lds {
    double* bval;           // [2][Lc + 1] the last DP row of the previous strip (double buffer)
    float* xs;              // [Lc][3]
    float* ys;              // [Lc][3]
    float* pts;             // [Lc][6] aligned pairs (x, y) of the alignment being searched
    uint32_t* trace;        // [Lc][W] 2-bit DP cell codes, W = ceil(Lc / 16)
    uint32_t* sets;         // [2][NW][64] each lane's cut sets (current, new), NW = ceil(Lc / 32)
    int* ixo;               // [Lc] compacted x -> slot index
    int* mbest;             // [Lc] invmap0
    int* minv;              // [Lc] invmap
    int* mdp;               // [Lc] DP output
    int* mkeep;             // [Lc] stage 3's best candidate
    unsigned char* ssx;     // [Lc]
    unsigned char* ssy;     // [Lc]
    unsigned char* bflag;   // [2][Lc + 1] diagonal flags of bval
    unsigned char* kept;    // [Lc]
};

// LDS bytes of each field in layout order, 8-byte aligned each
__host__ __device__ __forceinline__ size_t ta_lds_field(int Lc, int f) {
    const size_t n = (size_t)Lc, W = (n + 15) / 16, NW = (n + 31) / 32;
    size_t b = 0;
    switch (f) {
        case 0: b = sizeof(double) * 2 * (n + 1); break;    // bval
        case 1: case 2: b = sizeof(float) * 3 * n; break;   // xs, ys
        case 3: b = sizeof(float) * 6 * n; break;           // pts
        case 4: b = sizeof(uint32_t) * n * W; break;        // trace
        case 5: b = sizeof(uint32_t) * 2 * NW * 64; break;  // sets
        case 6: case 7: case 8: case 9: case 10: b = sizeof(int) * n; break;  // ixo, mbest, minv, mdp, mkeep
        case 11: case 12: case 14: b = n; break;            // ssx, ssy, kept
        case 13: b = 2 * (n + 1); break;                    // bflag
        default: break;
    }
    return (b + 7) & ~(size_t)7;
}

__host__ __device__ __forceinline__ size_t ta_lds_bytes(int Lc) {
    size_t o = 0;
    for (int f = 0; f < 15; ++f) o += ta_lds_field(Lc, f);
    return o;
}

__device__ __forceinline__ Lds ta_lds_at(int Lc, char* base) {
    size_t o = 0;
    Lds L;
    L.bval = (double*)(base + o); o += ta_lds_field(Lc, 0);
    L.xs = (float*)(base + o); o += ta_lds_field(Lc, 1);
    L.ys = (float*)(base + o); o += ta_lds_field(Lc, 2);
    L.pts = (float*)(base + o); o += ta_lds_field(Lc, 3);
    L.trace = (uint32_t*)(base + o); o += ta_lds_field(Lc, 4);
    L.sets = (uint32_t*)(base + o); o += ta_lds_field(Lc, 5);
    L.ixo = (int*)(base + o); o += ta_lds_field(Lc, 6);
    L.mbest = (int*)(base + o); o += ta_lds_field(Lc, 7);
    L.minv = (int*)(base + o); o += ta_lds_field(Lc, 8);
    L.mdp = (int*)(base + o); o += ta_lds_field(Lc, 9);
    L.mkeep = (int*)(base + o); o += ta_lds_field(Lc, 10);
    L.ssx = (unsigned char*)(base + o); o += ta_lds_field(Lc, 11);
    L.ssy = (unsigned char*)(base + o); o += ta_lds_field(Lc, 12);
    L.bflag = (unsigned char*)(base + o); o += ta_lds_field(Lc, 13);
    L.kept = (unsigned char*)(base + o);
    return L;
}

struct Xf {
    double R[3][3], t[3];
};

__device__ __forceinline__ void ta_identity(Xf& f) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        f.t[r] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) f.R[r][c] = r == c ? 1.0 : 0.0;
    }
}

// R x + t, in the program's order: t + u0 x0 + u1 x1 + u2 x2
__device__ __forceinline__ void ta_apply(const Xf& f, const double x[3], double o[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = f.t[r] + f.R[r][0] * x[0] + f.R[r][1] * x[1] + f.R[r][2] * x[2];
}

__device__ __forceinline__ double ta_d2(const Xf& f, const double x[3], const double y[3]) {
    double o[3];
    ta_apply(f, x, o);
    const double e0 = o[0] - y[0], e1 = o[1] - y[1], e2 = o[2] - y[2];
    return e0 * e0 + e1 * e1 + e2 * e2;
}

__device__ __forceinline__ double ta_term(double d2, double d02) { return 1.0 / (1.0 + d2 / d02); }

// the canonical rotation of a two-point fit (see the header)
__device__ __forceinline__ void ta_two_point(const double a[3], const double b[3], double R[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = r == c ? 1.0 : 0.0;
    const double na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
    if (!(na > 0.0 && nb > 0.0)) return;
    double ua[3], ub[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ua[k] = a[k] / na; ub[k] = b[k] / nb; }
    const double c = ua[0] * ub[0] + ua[1] * ub[1] + ua[2] * ub[2];
    if (1.0 + c <= 1e-12) {
        int k = 0;
        if (fabs(ua[1]) < fabs(ua[k])) k = 1;
        if (fabs(ua[2]) < fabs(ua[k])) k = 2;
        const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double n[3] = {ua[1] * e[2] - ua[2] * e[1], ua[2] * e[0] - ua[0] * e[2], ua[0] * e[1] - ua[1] * e[0]};
        const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
        for (int q = 0; q < 3; ++q) n[q] = n[q] / nn;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) R[r][q] = 2.0 * n[r] * n[q] - (r == q ? 1.0 : 0.0);
        return;
    }
    const double v[3] = {ua[1] * ub[2] - ua[2] * ub[1], ua[2] * ub[0] - ua[0] * ub[2], ua[0] * ub[1] - ua[1] * ub[0]};
    const double K[3][3] = {{0.0, -v[2], v[1]}, {v[2], 0.0, -v[0]}, {-v[1], v[0], 0.0}};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double kk = K[r][0] * K[0][q] + K[r][1] * K[1][q] + K[r][2] * K[2][q];
            R[r][q] = (r == q ? 1.0 : 0.0) + K[r][q] + kk / (1.0 + c);
        }
}

// proper least-squares fit y ~ R x + t of the pairs k < n with sel(k); get(k, x, y) loads pair k.  Both are called for k = 0 .. n-1
// in order, twice.
template <class Sel, class Get>
__device__ __forceinline__ void ta_fit(int n, Sel&& sel, Get&& get, Xf& f) {
    double cnt = 0.0, sx[3] = {0.0, 0.0, 0.0}, sy[3] = {0.0, 0.0, 0.0}, x0[3], y0[3], x1[3], y1[3];
    for (int k = 0; k < n; ++k) {
        if (!sel(k)) continue;
        double xv[3], yv[3];
        get(k, xv, yv);
        if (cnt == 0.0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { x0[c] = xv[c]; y0[c] = yv[c]; }
        } else if (cnt == 1.0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { x1[c] = xv[c]; y1[c] = yv[c]; }
        }
        cnt += 1.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { sx[c] += xv[c]; sy[c] += yv[c]; }
    }
    ta_identity(f);
    if (cnt == 0.0) return;
    double mx[3], my[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { mx[c] = sx[c] / cnt; my[c] = sy[c] / cnt; }
    if (cnt == 2.0) {
        const double a[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]}, b[3] = {y1[0] - y0[0], y1[1] - y0[1], y1[2] - y0[2]};
        ta_two_point(a, b, f.R);
    } else if (cnt >= 3.0) {
        double C[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        for (int k = 0; k < n; ++k) {
            if (!sel(k)) continue;
            double xv[3], yv[3];
            get(k, xv, yv);
#pragma unroll
            for (int c = 0; c < 3; ++c) { xv[c] -= mx[c]; yv[c] -= my[c]; }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) C[r][c] += xv[r] * yv[c];
        }
        double lam;
        kabsch_rotation(C, false, f.R, lam);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) f.t[r] = my[r] - (f.R[r][0] * mx[0] + f.R[r][1] * mx[1] + f.R[r][2] * mx[2]);
}

__device__ __forceinline__ void ta_three(double v, double& m0, double& m1, double& m2) {
    if (v < m0) { const double u = m0; m0 = v; v = u; }
    if (v < m1) { const double u = m1; m1 = v; v = u; }
    if (v < m2) m2 = v;
}

// score_fun8's raised cut: the least d + 0.5 m (m >= 0) with third < (d + 0.5 m)^2
__device__ __forceinline__ double ta_raise_d(double third, double d) {
    double m = floor((sqrt(third) - d) * 2.0) - 1.0;
    if (!(m > 0.0)) m = 0.0;
    for (int g = 0; g < 64 && !(third < (d + 0.5 * m) * (d + 0.5 * m)); ++g) m += 1.0;
    return d + 0.5 * m;
}

// get_score_fast's raised cut: t2 + 0.5 m for the least m >= 0 with third <= t2 + 0.5 m
__device__ __forceinline__ double ta_raise_sq(double third, double t2) {
    double m = ceil((third - t2) * 2.0) - 1.0;
    if (!(m > 0.0)) m = 0.0;
    for (int g = 0; g < 64 && !(third <= t2 + 0.5 * m); ++g) m += 1.0;
    for (int g = 0; g < 64 && m > 0.0 && third <= t2 + 0.5 * (m - 1.0); ++g) m -= 1.0;
    return t2 + 0.5 * m;
}

struct Par {
    double d0, d02, d0s, d8, d8sq, ddcc, lmin;
};

// get_score_fast over the n pairs get(k) (all taken), on this lane alone
template <class Get>
__device__ __forceinline__ double ta_quick(int n, const Par& P, Get&& get) {
    auto all = [](int) { return true; };
    Xf f1, f2, f3;
    ta_fit(n, all, get, f1);
    double s0 = 0.0, m0 = __builtin_inf(), m1 = m0, m2 = m0;
    const double t2a = P.d0s * P.d0s;
    int cnt = 0;
    for (int k = 0; k < n; ++k) {
        double xv[3], yv[3];
        get(k, xv, yv);
        const double d2 = ta_d2(f1, xv, yv);
        s0 += ta_term(d2, P.d02);
        cnt += d2 <= t2a;
        ta_three(d2, m0, m1, m2);
    }
    double thr = t2a;
    if (cnt < 3 && n > 3 && m2 <= 1e300) thr = ta_raise_sq(m2, t2a);
    int kept = 0;
    for (int k = 0; k < n; ++k) {
        double xv[3], yv[3];
        get(k, xv, yv);
        kept += ta_d2(f1, xv, yv) <= thr;
    }
    if (kept == n) return s0;
    ta_fit(n, [&](int k) { double xv[3], yv[3]; get(k, xv, yv); return ta_d2(f1, xv, yv) <= thr; }, get, f2);
    double s1 = 0.0;
    m0 = m1 = m2 = __builtin_inf();
    const double t2b = P.d0s * P.d0s + 1.0;
    cnt = 0;
    for (int k = 0; k < n; ++k) {
        double xv[3], yv[3];
        get(k, xv, yv);
        const double d2 = ta_d2(f2, xv, yv);
        s1 += ta_term(d2, P.d02);
        cnt += d2 <= t2b;
        ta_three(d2, m0, m1, m2);
    }
    double thr2 = t2b;
    if (cnt < 3 && n > 3 && m2 <= 1e300) thr2 = ta_raise_sq(m2, t2b);
    ta_fit(n, [&](int k) { double xv[3], yv[3]; get(k, xv, yv); return ta_d2(f2, xv, yv) <= thr2; }, get, f3);
    double s2 = 0.0;
    for (int k = 0; k < n; ++k) {
        double xv[3], yv[3];
        get(k, xv, yv);
        s2 += ta_term(ta_d2(f3, xv, yv), P.d02);
    }
    const double s = s1 > s0 ? s1 : s0;
    return s2 > s ? s2 : s;
}

__device__ __forceinline__ void ta_bcast(Xf& f, int src) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        f.t[r] = __shfl(f.t[r], src);
#pragma unroll
        for (int c = 0; c < 3; ++c) f.R[r][c] = __shfl(f.R[r][c], src);
    }
}

// seed lengths of TMscore8_search: n, n/2, ... while above min(4, n), then min(4, n) (at most five halvings): nl of them, the u-th
// is n >> u below nl - 1 and min(4, n) last
__device__ __forceinline__ int ta_seed_count(int n) {
    const int lmin = n < 4 ? n : 4;
    for (int m = 0; m < 5; ++m)
        if ((n >> m) <= lmin) return m + 1;
    return 6;
}

__device__ __forceinline__ int ta_seed_len(int n, int nl, int u) { return u < nl - 1 ? n >> u : (n < 4 ? n : 4); }

__device__ __forceinline__ int ta_start_count(int last, int step) { return last > 0 ? (last + step - 1) / step + 1 : 1; }

// TMscore8_search over the n pairs in L.pts (wave-wide; lanes take seeds).  d8sq < 0: every pair counts.  Returns the best score
// (uniform) and sets f to its transform; n == 0: 0, f unchanged.
__device__ __forceinline__ double ta_search(const Lds& L, int n, int step, double d8sq, double d0, double d0s, double lnorm, int lane, Xf& f) {
    if (n == 0) return 0.0;
    const float* pts = L.pts;
    const int NW = (n + 31) >> 5;
    uint32_t* S = L.sets;                   // [NW][64]
    uint32_t* Sn = L.sets + NW * 64;
    const int nl = ta_seed_count(n);
    int total = 0;
    for (int u = 0; u < nl; ++u) total += ta_start_count(n - ta_seed_len(n, nl, u), step);
    const double d02 = d0 * d0;
    auto get = [&](int k, double xv[3], double yv[3]) {
        load3d(pts + 6 * k, xv);
        load3d(pts + 6 * k + 3, yv);
    };
    double best = -1.0;
    long long bestc = LLONG_MAX;
    Xf bf;
    ta_identity(bf);
    for (int sd = lane; sd - lane < total; sd += 64) {
        if (sd >= total) continue;
        int ls = 0, s0 = 0, r = sd;
        for (int u = 0; u < nl; ++u) {
            const int lu = ta_seed_len(n, nl, u), last = n - lu, c = ta_start_count(last, step);
            if (r < c) {
                ls = lu;
                s0 = min(r * step, last);
                break;
            }
            r -= c;
        }
        for (int w = 0; w < NW; ++w) {
            const int lo = min(max(s0 - 32 * w, 0), 32), hi = min(max(s0 + ls - 32 * w, 0), 32);
            const uint32_t below_hi = hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u);
            const uint32_t below_lo = lo >= 32 ? 0xffffffffu : ((1u << lo) - 1u);
            S[w * 64 + lane] = below_hi & ~below_lo;
        }
        for (int it = 0; it < TA_CAND; ++it) {
            Xf g;
            uint32_t word = 0;
            auto sel = [&](int k) {
                if ((k & 31) == 0) word = S[(k >> 5) * 64 + lane];
                return ((word >> (k & 31)) & 1u) != 0u;
            };
            ta_fit(n, sel, get, g);
            const double d = it == 0 ? d0s - 1.0 : d0s + 1.0, dd = d * d;
            double sc = 0.0, m0 = __builtin_inf(), m1 = m0, m2 = m0;
            int cnt = 0;
            uint32_t acc = 0u;
            for (int k = 0; k < n; ++k) {
                double xv[3], yv[3];
                get(k, xv, yv);
                const double d2 = ta_d2(g, xv, yv);
                if (!(d8sq >= 0.0) || d2 <= d8sq) sc += ta_term(d2, d02);
                const bool in = d2 < dd;
                acc |= (uint32_t)in << (k & 31);
                cnt += in;
                ta_three(d2, m0, m1, m2);
                if ((k & 31) == 31 || k == n - 1) {
                    Sn[(k >> 5) * 64 + lane] = acc;
                    acc = 0u;
                }
            }
            sc = sc / lnorm;
            if (sc > best) {
                best = sc;
                bestc = (long long)sd * TA_CAND + it;
                bf = g;
            }
            if (it == TA_CAND - 1) break;
            if (cnt < 3 && n > 3 && m2 <= 1e300) {
                const double dm = ta_raise_d(m2, d), dm2 = dm * dm;
                cnt = 0;
                acc = 0u;
                for (int k = 0; k < n; ++k) {
                    double xv[3], yv[3];
                    get(k, xv, yv);
                    const bool in = ta_d2(g, xv, yv) < dm2;
                    acc |= (uint32_t)in << (k & 31);
                    cnt += in;
                    if ((k & 31) == 31 || k == n - 1) {
                        Sn[(k >> 5) * 64 + lane] = acc;
                        acc = 0u;
                    }
                }
            }
            bool same = it > 0;
            for (int w = 0; w < NW; ++w) {
                const uint32_t a = Sn[w * 64 + lane];
                same = same && a == S[w * 64 + lane];
                S[w * 64 + lane] = a;
            }
            if (same || cnt < 3) break;
        }
    }
    double wb = best;
    long long wc = bestc;
    wave_best(wb, wc);
    const unsigned long long hold = __ballot(wc != LLONG_MAX && bestc == wc);
    const int src = hold ? __ffsll((long long)hold) - 1 : 0;
    ta_bcast(bf, src);
    if (hold) f = bf;
    return wb;
}

// compact the pairs of the map m (over Ly) into L.pts in y order; returns their count (uniform)
__device__ __forceinline__ int ta_compact(const Lds& L, const int* m, int Ly, int lane) {
    int n = 0;
    for (int base = 0; base < Ly; base += 64) {
        const int j = base + lane;
        const int i = j < Ly ? m[j] : -1;
        const unsigned long long bal = __ballot(i >= 0);
        if (i >= 0) {
            const int pos = n + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                L.pts[6 * pos + c] = L.xs[3 * i + c];
                L.pts[6 * pos + 3 + c] = L.ys[3 * j + c];
            }
        }
        n += __popcll(bal);
    }
    ta_sync();
    return n;
}

__device__ __forceinline__ void ta_copy_map(int* dst, const int* src, int Ly, int lane) {
    for (int j = lane; j < Ly; j += 64) dst[j] = src[j];
    ta_sync();
}

// NWDP_TM (wave-wide).  mode 0: s = 1 / (1 + d^2 / d02) under f; 1: [ssx == ssy]; 2: mode 0 + 0.5 [ssx == ssy].  Writes y2x.
__device__ __forceinline__ void ta_dp(const Lds& L, int Lx, int Ly, int mode, const Xf& f, double d02, double gap, int* y2x, int lane) {
    const int W = (Ly + 15) >> 4;
    for (int j = lane; j <= Ly; j += 64) {
        L.bval[j] = 0.0;
        L.bflag[j] = 0;
    }
    for (int j = lane; j < Ly; j += 64) y2x[j] = -1;
    ta_sync();
    int buf = 0;
    for (int r0 = 0; r0 < Lx; r0 += 64) {
        const int i = r0 + 1 + lane, rows = min(64, Lx - r0);
        const bool row_ok = lane < rows;
        double xx[3] = {0.0, 0.0, 0.0};
        unsigned char sx = 0;
        if (row_ok) {
            double xv[3];
            load3d(L.xs + 3 * (i - 1), xv);
            if (mode != 1) ta_apply(f, xv, xx);
            sx = L.ssx[i - 1];
        }
        const double* bin = L.bval + buf * (Ly + 1);
        const unsigned char* fin = L.bflag + buf * (Ly + 1);
        double* bout = L.bval + (buf ^ 1) * (Ly + 1);
        unsigned char* fout = L.bflag + (buf ^ 1) * (Ly + 1);
        double cur = 0.0, prev_up = 0.0;
        bool curf = false;
        uint32_t acc = 0u;
        const int steps = Ly + rows - 1;
        for (int t = 0; t < steps; ++t) {
            double up = __shfl_up(cur, 1);
            bool upf = __shfl_up((int)curf, 1) != 0;
            const int j = t - lane + 1;
            const bool act = row_ok && j >= 1 && j <= Ly;
            if (lane == 0 && act) {
                up = bin[j];
                upf = fin[j] != 0;
            }
            if (act) {
                double s;
                if (mode == 1) {
                    s = sx == L.ssy[j - 1] ? 1.0 : 0.0;
                } else {
                    double yv[3];
                    load3d(L.ys + 3 * (j - 1), yv);
                    const double e0 = xx[0] - yv[0], e1 = xx[1] - yv[1], e2 = xx[2] - yv[2];
                    s = ta_term(e0 * e0 + e1 * e1 + e2 * e2, d02);
                    if (mode == 2 && sx == L.ssy[j - 1]) s = s + 0.5;
                }
                const double dd = prev_up + s;
                const double h = upf ? up + gap : up;
                const double v = curf ? cur + gap : cur;
                uint32_t code;
                if (dd >= h && dd >= v) {
                    cur = dd;
                    curf = true;
                    code = 0u;
                } else {
                    curf = false;
                    if (v >= h) { cur = v; code = 1u; }
                    else { cur = h; code = 2u; }
                }
                acc |= code << (2 * ((j - 1) & 15));
                if (((j - 1) & 15) == 15 || j == Ly) {
                    L.trace[(size_t)(i - 1) * W + ((j - 1) >> 4)] = acc;
                    acc = 0u;
                }
                if (lane == rows - 1) {
                    bout[j] = cur;
                    fout[j] = curf;
                }
            }
            prev_up = up;
        }
        if (lane == 0) {
            bout[0] = 0.0;
            fout[0] = 0;
        }
        buf ^= 1;
        ta_sync();
    }
    if (lane == 0) {
        int i = Lx, j = Ly;
        while (i > 0 && j > 0) {
            const uint32_t code = (L.trace[(size_t)(i - 1) * W + ((j - 1) >> 4)] >> (2 * ((j - 1) & 15))) & 3u;
            if (code == 0u) {
                y2x[j - 1] = i - 1;
                --i;
                --j;
            } else if (code == 1u) {
                --j;
            } else {
                --i;
            }
        }
    }
    ta_sync();
}

// make_sec for one residue
__device__ __forceinline__ unsigned char ta_sec(const float* xs, int L, int i) {
    if (i < 2 || i + 2 >= L) return 0;
    double p[5][3];
#pragma unroll
    for (int a = 0; a < 5; ++a) load3d(xs + 3 * (i - 2 + a), p[a]);
    auto dd = [&](int a, int b) {
        const double e0 = p[a][0] - p[b][0], e1 = p[a][1] - p[b][1], e2 = p[a][2] - p[b][2];
        return sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    };
    const double d13 = dd(0, 2), d14 = dd(0, 3), d15 = dd(0, 4), d24 = dd(1, 3), d25 = dd(1, 4), d35 = dd(2, 4);
    if (fabs(d15 - 6.37) < 2.1 && fabs(d14 - 5.18) < 2.1 && fabs(d25 - 5.18) < 2.1 && fabs(d13 - 5.45) < 2.1 &&
        fabs(d24 - 5.45) < 2.1 && fabs(d35 - 5.45) < 2.1)
        return 1;
    if (fabs(d15 - 13.0) < 1.42 && fabs(d14 - 10.4) < 1.42 && fabs(d25 - 10.4) < 1.42 && fabs(d13 - 6.1) < 1.42 &&
        fabs(d24 - 6.1) < 1.42 && fabs(d35 - 6.1) < 1.42)
        return 2;
    return d15 < 8.0 ? 3 : 0;
}

// find_max_frag on this lane (every lane computes the same): the first longest run [start, end]
__device__ __forceinline__ void ta_max_frag(const float* zs, int L, int& start, int& end) {
    const int r_min = min(4, L / 3);
    double f = 1.0;
    start = end = 0;
    for (int inc = 0; inc <= TA_FRAG_RAISES; ++inc) {
        const double dc = 4.25 * f, cut = dc * dc;
        int best = 0, bs = 0, be = 0, j = 1, st = 0;
        for (int i = 1; i < L; ++i) {
            double a[3], b[3];
            load3d(zs + 3 * (i - 1), a);
            load3d(zs + 3 * i, b);
            const double e0 = b[0] - a[0], e1 = b[1] - a[1], e2 = b[2] - a[2];
            if (e0 * e0 + e1 * e1 + e2 * e2 < cut) {
                ++j;
                if (i == L - 1) {
                    if (j > best) { best = j; bs = st; be = i; }
                    j = 1;
                }
            } else {
                if (j > best) { best = j; bs = st; be = i - 1; }
                j = 1;
                st = i;
            }
        }
        start = bs;
        end = be;
        if (best >= r_min) break;
        f *= 1.1;
    }
}

// gapless threading: shift q of [0, nsh) pairs y[yo + u] with x[xo + u], u < cnt; the shift's segment
struct Seg {
    int xo, yo, cnt;
};

// stage 1 / 5 candidates: y_j <-> xrun[j + k] (yrun == false; the x run starts at xs0, length lx) or yrun[j] <-> x[j + k]
__device__ __forceinline__ Seg ta_seg(int k, bool yrun, int run0, int lrun, int Lx, int Ly) {
    Seg s;
    const int j0 = k < 0 ? -k : 0;
    if (!yrun) {
        const int j1 = min(Ly, lrun - k);
        s.yo = j0;
        s.xo = run0 + j0 + k;
        s.cnt = max(j1 - j0, 0);
    } else {
        const int j1 = min(lrun, Lx - k);
        s.yo = run0 + j0;
        s.xo = j0 + k;
        s.cnt = max(j1 - j0, 0);
    }
    return s;
}

// threading over shifts n1 .. n2, lanes in parallel; the last of equal quick scores; writes the winner's map into m
__device__ __forceinline__ void ta_thread(const Lds& L, const Par& P, int n1, int n2, bool yrun, int run0, int lrun, int Lx, int Ly, int* m,
                          int lane) {
    double best = -__builtin_inf();
    long long bk = LLONG_MIN;
    for (int k = n1 + lane; k - lane <= n2; k += 64) {
        if (k > n2) continue;
        const Seg s = ta_seg(k, yrun, run0, lrun, Lx, Ly);
        const double sc = ta_quick(s.cnt, P, [&](int u, double xv[3], double yv[3]) {
            load3d(L.xs + 3 * (s.xo + u), xv);
            load3d(L.ys + 3 * (s.yo + u), yv);
        });
        if (sc >= best) { best = sc; bk = k; }
    }
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) {           // the largest (score, k): the last of equal scores
        const double s2 = __shfl_xor(best, msk);
        const long long k2 = __shfl_xor(bk, msk);
        if (s2 > best || (s2 == best && k2 > bk)) { best = s2; bk = k2; }
    }
    const Seg s = ta_seg((int)bk, yrun, run0, lrun, Lx, Ly);
    for (int j = lane; j < Ly; j += 64) m[j] = -1;
    ta_sync();
    for (int u = lane; u < s.cnt; u += 64) m[s.yo + u] = s.xo + u;
    ta_sync();
}

struct Stage {
    double tmmax;
    Xf f;
};

// detailed search (step 40, method 8) on the map m; sets the transform
__device__ __forceinline__ double ta_detailed(const Lds& L, const Par& P, const int* m, int Ly, int lane, Xf& f, int step = TA_STEP) {
    const int n = ta_compact(L, m, Ly, lane);
    const double sc = ta_search(L, n, step, P.d8sq, P.d0, P.d0s, P.lmin, lane, f);
    ta_sync();
    return sc;
}

// DP_iter: the best map goes to out; returns its score
__device__ __forceinline__ double ta_dp_iter(const Lds& L, const Par& P, int Lx, int Ly, int g0, int g1, int iters, int* out, int lane, Xf& f) {
    double best = -1.0, old = 0.0;
    for (int g = g0; g < g1; ++g) {
        const double gap = g == 0 ? -0.6 : 0.0;
        for (int it = 0; it < iters; ++it) {
            ta_dp(L, Lx, Ly, 0, f, P.d02, gap, L.mdp, lane);
            const double sc = ta_detailed(L, P, L.mdp, Ly, lane, f);
            if (sc > best) {
                best = sc;
                ta_copy_map(out, L.mdp, Ly, lane);
            }
            if (it > 0 && fabs(old - sc) < 0.000001) break;
            old = sc;
        }
    }
    return best;
}

__device__ __forceinline__ const float* ta_row(const float* base, int b, int N) { return base + (size_t)b * N * 3; }

__global__ __launch_bounds__(64) void tm_align_kernel(pf_tm_align_args a, int Lc) {
    extern __shared__ __align__(16) char ta_lds[];
    const Lds L = ta_lds_at(Lc, ta_lds);
    const int lane = threadIdx.x;
    const int p = blockIdx.x;
    const int N = a.N;
    const int bi = a.pairs[2 * p], bj = a.pairs[2 * p + 1];
    const bool valid = bi >= 0 && bi < a.Bx && bj >= 0 && bj < a.By;
    const float* X = ta_row(a.x, valid ? bi : 0, N);
    const float* Y = ta_row(a.y, valid ? bj : 0, N);
    const unsigned char* MX = a.mx + (size_t)(valid ? bi : 0) * N;
    const unsigned char* MY = a.my + (size_t)(valid ? bj : 0) * N;

    // lengths first: nothing is written to LDS beyond Lc
    int Lx = 0, Ly = 0;
    if (valid)
        for (int base = 0; base < N; base += 64) {
            const int k = base + lane;
            Lx += __popcll(__ballot(k < N && MX[k]));
            Ly += __popcll(__ballot(k < N && MY[k]));
        }
    const bool fits = Lx <= Lc && Ly <= Lc;
    const bool ok = valid && fits && Lx >= 3 && Ly >= 3;
    const float qnan = __int_as_float(0x7fc00000);
    if (!ok) {
        if (lane == 0) {
            a.tm[p] = qnan;
            a.tm_x[p] = qnan;
            a.rmsd[p] = qnan;
            a.n_aligned[p] = valid && !fits ? -1 : 0;
            a.len_x[p] = Lx;
            a.len_y[p] = Ly;
            if (a.rot) {
#pragma unroll
                for (int k = 0; k < 9; ++k) a.rot[(size_t)p * 9 + k] = k % 4 == 0 ? 1.0f : 0.0f;
#pragma unroll
                for (int k = 0; k < 3; ++k) a.trans[(size_t)p * 3 + k] = qnan;
            }
        }
        if (a.y2x)
            for (int k = lane; k < N; k += 64) {
                a.y2x[(size_t)p * N + k] = -1;
                a.kept[(size_t)p * N + k] = 0;
            }
        if (a.aligned)
            for (int k = lane; k < 3 * N; k += 64) a.aligned[(size_t)p * N * 3 + k] = qnan;
        return;
    }

    // compact both chains into LDS (index order)
    {
        int nx = 0, ny = 0;
        for (int base = 0; base < N; base += 64) {
            const int k = base + lane;
            const bool inx = k < N && MX[k], iny = k < N && MY[k];
            const unsigned long long bx = __ballot(inx), by = __ballot(iny);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (inx) {
                const int q = nx + __popcll(bx & below);
#pragma unroll
                for (int c = 0; c < 3; ++c) L.xs[3 * q + c] = X[(size_t)k * 3 + c];
                L.ixo[q] = k;
            }
            if (iny) {
                const int q = ny + __popcll(by & below);
#pragma unroll
                for (int c = 0; c < 3; ++c) L.ys[3 * q + c] = Y[(size_t)k * 3 + c];
            }
            nx += __popcll(bx);
            ny += __popcll(by);
        }
        ta_sync();
    }
    for (int i = lane; i < Lx; i += 64) L.ssx[i] = ta_sec(L.xs, Lx, i);
    for (int j = lane; j < Ly; j += 64) L.ssy[j] = ta_sec(L.ys, Ly, j);
    ta_sync();

    Par P;
    {
        const int lmin = min(Lx, Ly);
        double d0 = lmin <= 19 ? 0.168 : 1.24 * cbrt((double)lmin - 15.0) - 1.8;
        d0 += 0.8;
        P.d0 = d0;
        P.d02 = d0 * d0;
        P.d0s = d0 < 4.5 ? 4.5 : (d0 > 8.0 ? 8.0 : d0);
        P.d8 = 1.5 * pow((double)lmin, 0.3) + 3.5;
        P.d8sq = P.d8 * P.d8;
        P.ddcc = lmin <= 40 ? 0.1 : 0.4;
        P.lmin = lmin;
    }
    Xf f;
    ta_identity(f);
    double tmmax = -1.0;
    auto compete = [&](double tm, const int* m) {
        if (tm > tmmax) {
            tmmax = tm;
            ta_copy_map(L.mbest, m, Ly, lane);
        }
    };

    // 1. gapless threading
    {
        const int lmin = min(Lx, Ly);
        const int min_ali = max(lmin / 2, 5);
        const int n1 = -Ly + min_ali, n2 = Lx - min_ali;
        ta_thread(L, P, n1, n1 > n2 ? n1 : n2, false, 0, Lx, Lx, Ly, L.mbest, lane);
        const double tm = ta_detailed(L, P, L.mbest, Ly, lane, f);
        if (tm > tmmax) tmmax = tm;
        const double tm2 = ta_dp_iter(L, P, Lx, Ly, 0, 2, 30, L.minv, lane, f);
        compete(tm2, L.minv);
    }
    // 2. secondary structure
    {
        ta_dp(L, Lx, Ly, 1, f, 1.0, -1.0, L.minv, lane);
        const double tm = ta_detailed(L, P, L.minv, Ly, lane, f);
        compete(tm, L.minv);
        if (tm > tmmax * 0.2) {
            const double tm2 = ta_dp_iter(L, P, Lx, Ly, 0, 2, 30, L.minv, lane, f);
            compete(tm2, L.minv);
        }
    }
    // 3. local superposition
    {
        const int lmin = min(Lx, Ly);
        const double d01 = P.d0 + 1.5;
        const int jump_x = min(Lx > 250 ? 45 : Lx > 200 ? 35 : Lx > 150 ? 25 : 15, Lx / 3);
        const int jump_y = min(Ly > 250 ? 45 : Ly > 200 ? 35 : Ly > 150 ? 25 : 15, Ly / 3);
        double glmax = 0.0;
        bool found = false;
        for (int fr = 0; fr < 2; ++fr) {
            const int nf = fr == 0 ? min(20, lmin / 3) : min(100, lmin / 2);
            for (int i0 = 0; i0 < Lx - nf + 1; i0 += jump_x)
                for (int j0 = 0; j0 < Ly - nf + 1; j0 += jump_y) {
                    Xf g;
                    ta_fit(nf, [](int) { return true; },
                           [&](int k, double xv[3], double yv[3]) {
                               load3d(L.xs + 3 * (i0 + k), xv);
                               load3d(L.ys + 3 * (j0 + k), yv);
                           },
                           g);
                    ta_dp(L, Lx, Ly, 0, g, d01 * d01, 0.0, L.mdp, lane);
                    const int n = ta_compact(L, L.mdp, Ly, lane);
                    const double gl = ta_quick(n, P, [&](int k, double xv[3], double yv[3]) {
                        load3d(L.pts + 6 * k, xv);
                        load3d(L.pts + 6 * k + 3, yv);
                    });
                    ta_sync();
                    if (gl > glmax) {
                        glmax = gl;
                        found = true;
                        ta_copy_map(L.mkeep, L.mdp, Ly, lane);
                    }
                }
        }
        if (found) {
            ta_copy_map(L.minv, L.mkeep, Ly, lane);
            const double tm = ta_detailed(L, P, L.minv, Ly, lane, f);
            compete(tm, L.minv);
            if (tm > tmmax * P.ddcc) {
                const double tm2 = ta_dp_iter(L, P, Lx, Ly, 0, 2, 2, L.minv, lane, f);
                compete(tm2, L.minv);
            }
        }
    }
    // 4. secondary structure plus superposition
    {
        const double d01 = P.d0 + 1.5;
        const int n = ta_compact(L, L.mbest, Ly, lane);
        Xf g;
        ta_fit(n, [](int) { return true; },
               [&](int k, double xv[3], double yv[3]) {
                   load3d(L.pts + 6 * k, xv);
                   load3d(L.pts + 6 * k + 3, yv);
               },
               g);
        ta_sync();
        ta_dp(L, Lx, Ly, 2, g, d01 * d01, -1.0, L.minv, lane);
        const double tm = ta_detailed(L, P, L.minv, Ly, lane, f);
        compete(tm, L.minv);
        if (tm > tmmax * P.ddcc) {
            const double tm2 = ta_dp_iter(L, P, Lx, Ly, 0, 2, 30, L.minv, lane, f);
            compete(tm2, L.minv);
        }
    }
    // 5. fragment gapless threading
    {
        int xs0, xe0, ys0, ye0;
        ta_max_frag(L.xs, Lx, xs0, xe0);
        ta_max_frag(L.ys, Ly, ys0, ye0);
        const int lxf = xe0 - xs0 + 1, lyf = ye0 - ys0 + 1;
        const bool use_x = lxf < lyf || (lxf == lyf && Lx <= Ly);
        int lfr = min(lxf, lyf), run0 = use_x ? xs0 : ys0;
        const int L0 = min(Lx, Ly);
        if (lfr == L0) {
            const int t0 = (int)(L0 * 0.1), t1 = (int)(L0 * 0.89);
            run0 += t0;
            lfr = t1 - t0 + 1;
        }
        int n1, n2;
        if (use_x) {
            const int min_ali = max((int)(min(lfr, Ly) / 2.5), 3);
            n1 = -Ly + min_ali;
            n2 = lfr - min_ali;
        } else {
            const int min_ali = max((int)(min(Lx, lfr) / 2.5), 3);
            n1 = -lfr + min_ali;
            n2 = Lx - min_ali;
        }
        if (n1 <= n2) ta_thread(L, P, n1, n2, !use_x, run0, lfr, Lx, Ly, L.minv, lane);
        const double tm = ta_detailed(L, P, L.minv, Ly, lane, f);
        compete(tm, L.minv);
        if (tm > tmmax * P.ddcc) {
            const double tm2 = ta_dp_iter(L, P, Lx, Ly, 1, 2, 2, L.minv, lane, f);
            compete(tm2, L.minv);
        }
    }

    // 6. final: the step-1 search, the pairs within score_d8, rmsd, tm_x and tm
    ta_detailed(L, P, L.mbest, Ly, lane, f, 1);
    int n8 = 0;
    for (int base = 0; base < Ly; base += 64) {
        const int j = base + lane;
        const int i = j < Ly ? L.mbest[j] : -1;
        bool keep = false;
        double xv[3], yv[3];
        if (i >= 0) {
            load3d(L.xs + 3 * i, xv);
            load3d(L.ys + 3 * j, yv);
            keep = sqrt(ta_d2(f, xv, yv)) <= P.d8;
        }
        if (j < Ly) L.kept[j] = keep;
        const unsigned long long bal = __ballot(keep);
        if (keep) {
            const int pos = n8 + __popcll(bal & ((1ull << lane) - 1ull));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                L.pts[6 * pos + c] = (float)xv[c];
                L.pts[6 * pos + 3 + c] = (float)yv[c];
            }
        }
        n8 += __popcll(bal);
    }
    ta_sync();
    double rmsd = qnan;
    if (n8 > 0) {
        auto getp = [&](int k, double xv[3], double yv[3]) {
            load3d(L.pts + 6 * k, xv);
            load3d(L.pts + 6 * k + 3, yv);
        };
        Xf g;
        ta_fit(n8, [](int) { return true; }, getp, g);
        double e = 0.0;
        for (int k = 0; k < n8; ++k) {
            double xv[3], yv[3];
            getp(k, xv, yv);
            e += ta_d2(g, xv, yv);
        }
        rmsd = sqrt(e / n8);
    }
    double tm_x = 0.0, tm_y = 0.0;
    for (int c = 0; c < 2; ++c) {
        const int Ln = c == 0 ? Lx : Ly;
        double d0 = Ln <= 21 ? 0.5 : 1.24 * cbrt((double)Ln - 15.0) - 1.8;
        if (d0 < 0.5) d0 = 0.5;
        const double d0s = d0 < 4.5 ? 4.5 : (d0 > 8.0 ? 8.0 : d0);
        const double sc = ta_search(L, n8, 1, -1.0, d0, d0s, Ln, lane, f);
        if (c == 0) tm_x = sc;
        else tm_y = sc;
        ta_sync();
    }

    // outputs
    if (lane == 0) {
        a.tm[p] = (float)tm_y;
        a.tm_x[p] = (float)tm_x;
        a.rmsd[p] = (float)rmsd;
        a.n_aligned[p] = n8;
        a.len_x[p] = Lx;
        a.len_y[p] = Ly;
        if (a.rot) {
#pragma unroll
            for (int k = 0; k < 9; ++k) a.rot[(size_t)p * 9 + k] = (float)f.R[k / 3][k % 3];
#pragma unroll
            for (int k = 0; k < 3; ++k) a.trans[(size_t)p * 3 + k] = (float)f.t[k];
        }
    }
    if (a.y2x) {
        int ny = 0;
        for (int base = 0; base < N; base += 64) {
            const int k = base + lane;
            const bool iny = k < N && MY[k];
            const unsigned long long by = __ballot(iny);
            int o = -1, kp = 0;
            if (iny) {
                const int j = ny + __popcll(by & ((1ull << lane) - 1ull));
                const int i = L.mbest[j];
                o = i >= 0 ? L.ixo[i] : -1;
                kp = L.kept[j];
            }
            if (k < N) {
                a.y2x[(size_t)p * N + k] = o;
                a.kept[(size_t)p * N + k] = (unsigned char)kp;
            }
            ny += __popcll(by);
        }
    }
    if (a.aligned)
        for (int k = lane; k < N; k += 64) {
            double xv[3], o[3];
            load3d(X + (size_t)k * 3, xv);
            ta_apply(f, xv, o);
#pragma unroll
            for (int r = 0; r < 3; ++r) a.aligned[((size_t)p * N + k) * 3 + r] = (float)o[r];
        }
}

}  // namespace

extern "C" int pf_tm_align_lds_bytes(int max_len) {
    if (max_len < 1 || max_len > PF_TM_ALIGN_MAX_N) return 0;
    return (int)ta_lds_bytes(max_len);
}

extern "C" int pf_tm_align_fwd(const pf_tm_align_args* a, pf_stream_t stream) {
    if (!a || !a->x || !a->y || !a->mx || !a->my || !a->pairs || !a->tm || !a->tm_x || !a->rmsd || !a->n_aligned || !a->len_x ||
        !a->len_y || a->Bx <= 0 || a->By <= 0 || a->N <= 0 || a->P < 0 || a->max_len < 0 || (!a->rot != !a->trans) ||
        (!a->y2x != !a->kept))
        return PF_E_BADARG;
    if (a->N > PF_TM_ALIGN_MAX_N) return PF_E_TOOLARGE;
    if (a->P == 0) return 0;
    const int Lc = a->max_len > 0 && a->max_len < a->N ? a->max_len : a->N;
    const size_t lds = ta_lds_bytes(Lc);
    static PfOncePerDevice attr;
    if (lds > 64 * 1024 && attr.first())
        (void)hipFuncSetAttribute((const void*)tm_align_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(tm_align_kernel, dim3((unsigned)a->P), dim3(64), lds, (hipStream_t)stream, *a, Lc);
    PF_CHECK_LAUNCH();
    return 0;
}
