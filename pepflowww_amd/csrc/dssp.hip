// pf_dssp_fwd -- DSSP secondary structure (Kabsch & Sander, Biopolymers 22, 2577, 1983) of a batch of chain slots, with the
// conventions of DSSP 2.x, in fp64 from the fp32 coordinates.  8-state codes numbered as SSTRUCT_SYMB_TO_INDEX of
// pepflow/modules/protein/dssp.py: H 0, B 1, E 2, G 3, I 4, T 5, S 6, '-' 7; 255 where mask is false.
//
// Conventions (tests/dssp_oracle.py restates them in numpy):
//   Breaks    a segment starts at 0 and at i when mask is false on i - 1 or i, the chain ids differ, or |C(i-1) - N(i)| > 2.5 A.
//   Hydrogen  H(i) = N(i) + unit(C(i-1) - O(i-1)) x 1 A.  The first residue of a segment and prolines (aa == pro) are not donors.
//   Energy    E = 0.084 * 332 * (1/r_ON + 1/r_CH - 1/r_OH - 1/r_CN) kcal/mol between donor d (N, H) and acceptor a (C, O); -9.9 if
//             one of the four distances is < 0.5 A, and never below -9.9.  Computed only where CA-CA < 9 A, a != d, a != d - 1,
//             both unmasked.  Not rounded to 0.001 (DSSP's compatibility rounding).
//   H-bond    each donor keeps its two lowest energies below 0, ties to the lower acceptor index (DSSP's scan order); donor d
//             bonds acceptor a when a is one of them with E < -0.5.
//   Turns     an n-turn at i (n = 3, 4, 5): a bond from donor i + n to acceptor i, no break from i to i + n.
//   Bridges   (i, j), j >= i + 3, no break across i - 1 .. i + 1 nor j - 1 .. j + 1.  Parallel (tested first): bond(i+1 -> j) and
//             bond(j -> i-1), or bond(j+1 -> i) and bond(i -> j-1).  Antiparallel: bond(i+1 -> j-1) and bond(j+1 -> i-1), or
//             bond(j -> i) and bond(i -> j).
//   Ladders   a bridge continues the ladder of (i-1, j-1) (parallel) or (i-1, j+1) (antiparallel) of its type.  Bulges: in order
//             of the first i (ties: first j), each live ladder X takes every later live ladder Y of its type with gap_i = ib(Y) -
//             ie(X) in 1..5, gap_j = jb(Y) - je(X) (parallel) or jb(X) - je(Y) (antiparallel) >= 0, one gap < 3 and the other
//             < 6 (DSSP 2.x), and no break in the joined spans (DSSP 2.x only compares chain ids there).  A ladder of more than
//             one bridge gives E over both of its spans, bulges included; one of a single bridge gives B; B never replaces E.
//   Helices   after the bridges: H on i .. i+3 where 4-turns start at i-1 and i (over E and B); then G on i .. i+2 where 3-turns
//             start at i-1 and i, if all three are '-' or G; then I on i .. i+4 from 5-turns, if all five are '-' or I, or H
//             (PF_DSSP_PI_PRECEDENCE, DSSP >= 2.1).  T on a residue still '-' strictly inside an n-turn; S on one still '-'
//             whose kappa > 70 degrees: the angle between CA(i) - CA(i-2) and CA(i+2) - CA(i), no break from i-2 to i+2.
//
// One workgroup per chain slot, LDS sized by N (93 B per residue): 64 threads up to N = 64, 128 up to 128, then 256.  Stages,
// block barriers between them: coordinates into LDS; breaks and segment ids (one wave, ballot scan); a thread per donor scans all
// acceptors (LDS broadcast reads) for its two best and the bend at its residue; a thread per residue finds its turns and its
// bridges (j > i; at most 8, from the bonds of i and i + 1); a thread per bridge that starts a ladder walks it; one thread joins
// ladders across bulges in order; a thread per ladder marks its spans; a thread per residue runs the helix, T and S passes.
#include <climits>

#include "common.h"
#include "../../include/pepflow_hip.h"

namespace {

constexpr int SS_H = 0, SS_B = 1, SS_E = 2, SS_G = 3, SS_I = 4, SS_T = 5, SS_S = 6, SS_LOOP = 7, SS_MASKED = 255;
constexpr double Q = 0.084 * 332.0;
constexpr double HB_MAX = -0.5, HB_MIN = -9.9, MIN_DIST = 0.5, CA_CUT = 9.0, CN_BREAK = 2.5, BEND_DEG = 70.0;
constexpr double RAD_TO_DEG = 180.0 / 3.141592653589793;
constexpr int SLOTS = 8;                    // bridges (i, j > i) of residue i: j is a or a + 1 for a bonded acceptor of i or i + 1
constexpr int LDS_PER_RES = 93;

struct Lds {
    float* xyz;             // [N][12] N, CA, C, O; after the energy stage the same bytes hold short lad[N][SLOTS][3]
    short* acc;             // [N][2] the two best acceptors
    short* seg;             // [N] segment id
    short* brj;             // [N][SLOTS] bridge partner j, ascending
    unsigned char* brf;     // [N][SLOTS] 0 parallel, 1 antiparallel
    unsigned char* lf;      // [N][SLOTS] bit 0: a live ladder starts at this bridge, bit 1: it has more than one bridge
    unsigned char* st;      // [N] bit 0 unmasked, bit 1 a segment starts here
    unsigned char* fl;      // [N] bit 0 / 1: acc[0] / acc[1] is a bond, bit 2: bend
    unsigned char* tf;      // [N] bit n - 3: an n-turn starts here
    unsigned char* nbr;     // [N] bridges in brj
    unsigned char* ss;      // [N]
    unsigned char* cov0;    // [N] covered by a ladder of > 1 bridge, then by a G span
    unsigned char* cov1;    // [N] covered by a single bridge, then by an I span
};

__device__ __forceinline__ Lds dssp_carve(unsigned char* p, int N) {
    Lds s;
    s.xyz = reinterpret_cast<float*>(p);
    s.acc = reinterpret_cast<short*>(p + 48 * N);
    s.seg = reinterpret_cast<short*>(p + 52 * N);
    s.brj = reinterpret_cast<short*>(p + 54 * N);
    unsigned char* q = p + 70 * N;
    s.brf = q; q += SLOTS * N;
    s.lf = q; q += SLOTS * N;
    s.st = q; q += N;
    s.fl = q; q += N;
    s.tf = q; q += N;
    s.nbr = q; q += N;
    s.ss = q; q += N;
    s.cov0 = q; q += N;
    s.cov1 = q;
    return s;
}

__device__ __forceinline__ void ld3(const float* xyz, int k, int atom, double v[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = xyz[12 * k + 3 * atom + c];
}

__device__ __forceinline__ double dist(const double p[3], const double q[3]) {
    const double x = p[0] - q[0], y = p[1] - q[1], z = p[2] - q[2];
    return sqrt((x * x + y * y) + z * z);
}

// donor d to acceptor q
__device__ __forceinline__ bool dssp_bond(const Lds& s, int N, int d, int q) {
    if (d < 0 || d >= N) return false;
    const unsigned char f = s.fl[d];
    return (s.acc[2 * d] == q && (f & 1)) || (s.acc[2 * d + 1] == q && (f & 2));
}

// is (i, j) a bridge of this type
__device__ __forceinline__ bool dssp_has_bridge(const Lds& s, int N, int i, int j, int type) {
    if (i < 0 || i >= N) return false;
    const int nb = s.nbr[i];
    for (int u = 0; u < nb; ++u)
        if (s.brj[SLOTS * i + u] == j && s.brf[SLOTS * i + u] == type) return true;
    return false;
}

__global__ __launch_bounds__(256) void dssp_kernel(pf_dssp_args a) {
    extern __shared__ __align__(16) unsigned char dssp_lds[];
    const int N = a.N, tid = threadIdx.x, nt = blockDim.x;
    const size_t b = blockIdx.x;
    const Lds s = dssp_carve(dssp_lds, N);
    const unsigned char* M = a.mask + b * N;
    const int64_t* CH = a.chain ? a.chain + b * N : nullptr;
    const int64_t* AA = a.aa ? a.aa + b * N : nullptr;
    const float* P = a.pos + b * N * a.n_atoms * 3;

    for (int k = tid; k < N; k += nt) {
        const float* p = P + (size_t)k * a.n_atoms * 3;
#pragma unroll
        for (int c = 0; c < 12; ++c) s.xyz[12 * k + c] = p[c];
    }
    __syncthreads();

    // breaks and segment ids: wave 0, a ballot scan over chunks of 64
    if (tid < 64) {
        int run = -1;
        for (int base = 0; base < N; base += 64) {
            const int k = base + tid;
            bool v = false, brk = true;
            if (k < N) {
                v = M[k] != 0;
                if (k > 0 && v && M[k - 1] && (!CH || CH[k - 1] == CH[k])) {
                    double c[3], n[3];
                    ld3(s.xyz, k - 1, 2, c);
                    ld3(s.xyz, k, 0, n);
                    brk = dist(c, n) > CN_BREAK;
                }
            }
            const unsigned long long bal = __ballot(k < N && brk);
            if (k < N) {
                s.seg[k] = (short)(run + __popcll(bal & ((2ull << tid) - 1ull)));
                s.st[k] = (unsigned char)((v ? 1 : 0) | (brk ? 2 : 0));
            }
            run += __popcll(bal);
        }
    }
    __syncthreads();

    // H-bond energies: a thread per donor, every acceptor in turn; the bend of the same residue
    for (int d = tid; d < N; d += nt) {
        int a0 = -1, a1 = -1;
        double e0 = 0.0, e1 = 0.0;
        const unsigned char sd = s.st[d];
        if ((sd & 1) && !(sd & 2) && !(AA && AA[d] == a.pro)) {
            double n[3], ca[3], h[3], cp[3], op[3];
            ld3(s.xyz, d, 0, n);
            ld3(s.xyz, d, 1, ca);
            ld3(s.xyz, d - 1, 2, cp);
            ld3(s.xyz, d - 1, 3, op);
            const double v[3] = {cp[0] - op[0], cp[1] - op[1], cp[2] - op[2]};
            const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) h[c] = n[c] + v[c] / len;
            for (int q = 0; q < N; ++q) {
                if (!(s.st[q] & 1) || q == d || q == d - 1) continue;
                double caq[3];
                ld3(s.xyz, q, 1, caq);
                if (!(dist(ca, caq) < CA_CUT)) continue;
                double cq[3], oq[3];
                ld3(s.xyz, q, 2, cq);
                ld3(s.xyz, q, 3, oq);
                const double r_on = dist(oq, n), r_ch = dist(cq, h), r_oh = dist(oq, h), r_cn = dist(cq, n);
                double e;
                if (r_on < MIN_DIST || r_ch < MIN_DIST || r_oh < MIN_DIST || r_cn < MIN_DIST) {
                    e = HB_MIN;
                } else {
                    e = Q * (((1.0 / r_on + 1.0 / r_ch) - 1.0 / r_oh) - 1.0 / r_cn);
                    if (e < HB_MIN) e = HB_MIN;
                }
                if (e < e0) {
                    a1 = a0; e1 = e0;
                    a0 = q; e0 = e;
                } else if (e < e1) {
                    a1 = q; e1 = e;
                }
            }
        }
        bool bend = false;
        if (d >= 2 && d + 2 < N && s.seg[d - 2] == s.seg[d + 2]) {
            double pm[3], p0[3], pp[3];
            ld3(s.xyz, d - 2, 1, pm);
            ld3(s.xyz, d, 1, p0);
            ld3(s.xyz, d + 2, 1, pp);
            const double u[3] = {p0[0] - pm[0], p0[1] - pm[1], p0[2] - pm[2]};
            const double w[3] = {pp[0] - p0[0], pp[1] - p0[1], pp[2] - p0[2]};
            const double x = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) * ((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
            const double c = x > 0.0 ? ((u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]) / sqrt(x) : 0.0;
            bend = acos(fmin(1.0, fmax(-1.0, c))) * RAD_TO_DEG > BEND_DEG;
        }
        s.acc[2 * d] = (short)a0;
        s.acc[2 * d + 1] = (short)a1;
        s.fl[d] = (unsigned char)((a0 >= 0 && e0 < HB_MAX ? 1 : 0) | (a1 >= 0 && e1 < HB_MAX ? 2 : 0) | (bend ? 4 : 0));
        if (a.hb_acc) {
            a.hb_acc[(b * N + d) * 2] = a0;
            a.hb_acc[(b * N + d) * 2 + 1] = a1;
            a.hb_energy[(b * N + d) * 2] = (float)e0;
            a.hb_energy[(b * N + d) * 2 + 1] = (float)e1;
        }
    }
    __syncthreads();

    // turns and bridges: a thread per residue i, bridges (i, j > i) in ascending j
    for (int i = tid; i < N; i += nt) {
        unsigned char t = 0;
        for (int n = 3; n <= 5; ++n)
            if (i + n < N && s.seg[i] == s.seg[i + n] && dssp_bond(s, N, i + n, i)) t |= (unsigned char)(1 << (n - 3));
        s.tf[i] = t;
        s.cov0[i] = 0;
        s.cov1[i] = 0;
        int cnt = 0;
        if (i >= 1 && i + 1 < N && s.seg[i - 1] == s.seg[i + 1]) {
            int cand[8];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int r = i + 1 - u;                            // i + 1: j = a (parallel), a + 1 (antiparallel); i: a + 1, a
                const bool ok0 = s.fl[r] & 1, ok1 = (s.fl[r] >> 1) & 1;
                const int x0 = ok0 ? s.acc[2 * r] : -1, x1 = ok1 ? s.acc[2 * r + 1] : -1;
                cand[4 * u] = x0;
                cand[4 * u + 1] = x0 >= 0 ? x0 + 1 : -1;
                cand[4 * u + 2] = x1;
                cand[4 * u + 3] = x1 >= 0 ? x1 + 1 : -1;
            }
            int last = -1;
            for (int r = 0; r < 8; ++r) {
                int j = INT_MAX;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (cand[u] > last && cand[u] < j) j = cand[u];
                if (j == INT_MAX) break;
                last = j;
                if (j < i + 3 || j + 1 >= N || s.seg[j - 1] != s.seg[j + 1]) continue;
                int type = -1;
                if ((dssp_bond(s, N, i + 1, j) && dssp_bond(s, N, j, i - 1)) || (dssp_bond(s, N, j + 1, i) && dssp_bond(s, N, i, j - 1)))
                    type = 0;
                else if ((dssp_bond(s, N, i + 1, j - 1) && dssp_bond(s, N, j + 1, i - 1)) || (dssp_bond(s, N, j, i) && dssp_bond(s, N, i, j)))
                    type = 1;
                if (type >= 0) {
                    s.brj[SLOTS * i + cnt] = (short)j;
                    s.brf[SLOTS * i + cnt] = (unsigned char)type;
                    ++cnt;
                }
            }
        }
        s.nbr[i] = (unsigned char)cnt;
    }
    __syncthreads();

    // ladders: a thread per residue walks each ladder that starts at one of its bridges
    short* lad = reinterpret_cast<short*>(s.xyz);                   // [N][SLOTS][3]: ie, jb, je
    for (int i = tid; i < N; i += nt) {
        const int nb = s.nbr[i];
        for (int q = 0; q < nb; ++q) {
            const int sl = SLOTS * i + q, j = s.brj[sl], type = s.brf[sl], dj = type ? -1 : 1;
            unsigned char f = 0;
            if (!dssp_has_bridge(s, N, i - 1, j - dj, type)) {
                int ci = i, cj = j, cnt = 1;
                while (dssp_has_bridge(s, N, ci + 1, cj + dj, type)) {
                    ++ci;
                    cj += dj;
                    ++cnt;
                }
                lad[3 * sl] = (short)ci;
                lad[3 * sl + 1] = (short)(type ? cj : j);
                lad[3 * sl + 2] = (short)(type ? j : cj);
                f = (unsigned char)(1 | (cnt > 1 ? 2 : 0));
            }
            s.lf[sl] = f;
        }
    }
    __syncthreads();

    // bulges: one thread, the ladders in order of (first i, first j)
    if (tid == 0)
        for (int i = 0; i < N; ++i) {
            const int nb = s.nbr[i];
            for (int q = 0; q < nb; ++q) {
                const int sx = SLOTS * i + q;
                unsigned char fx = s.lf[sx];
                if (!(fx & 1)) continue;
                const int type = s.brf[sx];
                int iex = lad[3 * sx], jbx = lad[3 * sx + 1], jex = lad[3 * sx + 2];
                for (int i2 = i; i2 < N && i2 - iex < 6; ++i2) {
                    const int nb2 = s.nbr[i2];
                    for (int q2 = i2 == i ? q + 1 : 0; q2 < nb2; ++q2) {
                        const int sy = SLOTS * i2 + q2;
                        if (!(s.lf[sy] & 1) || s.brf[sy] != type) continue;
                        const int iey = lad[3 * sy], jby = lad[3 * sy + 1], jey = lad[3 * sy + 2];
                        const int gi = i2 - iex, gj = type ? jbx - jey : jby - jex;
                        if (gi < 1 || gj < 0 || !((gj < 6 && gi < 3) || gj < 3)) continue;
                        if (s.seg[i] != s.seg[max(iex, iey)] || s.seg[min(jbx, jby)] != s.seg[max(jex, jey)]) continue;
                        iex = iey;
                        if (type) jbx = jby;
                        else jex = jey;
                        fx |= 2;
                        s.lf[sy] = 0;
                    }
                }
                lad[3 * sx] = (short)iex;
                lad[3 * sx + 1] = (short)jbx;
                lad[3 * sx + 2] = (short)jex;
                s.lf[sx] = fx;
            }
        }
    __syncthreads();

    // E / B spans: every writer of a byte stores the same 1
    for (int i = tid; i < N; i += nt) {
        const int nb = s.nbr[i];
        for (int q = 0; q < nb; ++q) {
            const int sl = SLOTS * i + q;
            const unsigned char f = s.lf[sl];
            if (!(f & 1)) continue;
            unsigned char* cov = (f & 2) ? s.cov0 : s.cov1;
            for (int k = i; k <= lad[3 * sl]; ++k) cov[k] = 1;
            for (int k = lad[3 * sl + 1]; k <= lad[3 * sl + 2]; ++k) cov[k] = 1;
        }
    }
    __syncthreads();

    // H over the bridges
    for (int k = tid; k < N; k += nt) {
        unsigned char c = s.cov0[k] ? SS_E : (s.cov1[k] ? SS_B : SS_LOOP);
        for (int i = max(1, k - 3); i <= k; ++i)
            if ((s.tf[i - 1] & 2) && (s.tf[i] & 2)) c = SS_H;
        s.ss[k] = c;
    }
    __syncthreads();
    // G on free spans
    for (int k = tid; k < N; k += nt) {
        bool g = false;
        for (int i = max(1, k - 2); i <= k && !g; ++i)
            if ((s.tf[i - 1] & 1) && (s.tf[i] & 1))
                g = s.ss[i] == SS_LOOP && s.ss[i + 1] == SS_LOOP && s.ss[i + 2] == SS_LOOP;
        s.cov0[k] = g;
    }
    __syncthreads();
    for (int k = tid; k < N; k += nt)
        if (s.cov0[k]) s.ss[k] = SS_G;
    __syncthreads();
    // I on spans of '-' (and H under pi precedence)
    for (int k = tid; k < N; k += nt) {
        bool pi = false;
        for (int i = max(1, k - 4); i <= k && !pi; ++i)
            if ((s.tf[i - 1] & 4) && (s.tf[i] & 4)) {
                bool free = true;
                for (int m = i; m <= i + 4; ++m) {
                    const unsigned char c = s.ss[m];
                    free = free && (c == SS_LOOP || (PF_DSSP_PI_PRECEDENCE && c == SS_H));
                }
                pi = free;
            }
        s.cov1[k] = pi;
    }
    __syncthreads();
    // T, S, mask, store
    for (int k = tid; k < N; k += nt) {
        unsigned char c = s.cov1[k] ? (unsigned char)SS_I : s.ss[k];
        if (c == SS_LOOP) {
            bool turn = false;
            for (int n = 3; n <= 5; ++n)
                for (int m = 1; m < n; ++m) turn = turn || (k - m >= 0 && ((s.tf[k - m] >> (n - 3)) & 1));
            if (turn) c = SS_T;
            else if (s.fl[k] & 4) c = SS_S;
        }
        if (!(s.st[k] & 1)) c = SS_MASKED;
        a.ss[b * N + k] = c;
    }
}

}  // namespace

extern "C" int pf_dssp_fwd(const pf_dssp_args* a, pf_stream_t stream) {
    if (!a || !a->pos || !a->mask || !a->ss || a->B < 0 || a->N < 0 || a->n_atoms < 4 || (!a->hb_acc != !a->hb_energy))
        return PF_E_BADARG;
    if (a->N > PF_DSSP_MAX_N) return PF_E_TOOLARGE;
    if (a->B == 0 || a->N == 0) return 0;
    const int threads = a->N <= 64 ? 64 : (a->N <= 128 ? 128 : 256);
    const size_t lds = ((size_t)LDS_PER_RES * a->N + 15) & ~(size_t)15;
    hipLaunchKernelGGL(dssp_kernel, dim3((unsigned)a->B), dim3(threads), lds, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
