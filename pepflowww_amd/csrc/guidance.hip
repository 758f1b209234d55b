// Guided sampling: C-alpha potentials that steer the translation prediction of one sampler step (pf_guidance_fwd; formulas and
// conventions: include/pepflow_hip.h).  The reference has no such call; the potentials are written from their formulas.
//
// One workgroup of 256 threads per sample.  The sample's positions (pred_trans on movable rows, trans1 elsewhere) and row classes are
// staged in LDS once; everything after that reads LDS.  Accumulation is i-centric: a thread owns the rows i = tid, tid + 256, ... and
// sums, for each of them, over the partners j in ascending order, over the hot spots and over the restraint list -- no atomics, and
// the block sums are eval_dev.h's fixed tree, so two runs give the same bits, and a sample gives the same bits in any batch and at
// any padded length (rows without res_mask are skipped, they add nothing to any sum).
// The hot-spot term takes two passes with a barrier between them: the first lets a thread own hot spots j and leaves the soft-min
// s_j and the pull max(0, s_j - r) in LDS; the second lets each peptide row gather from them.  s_j carries its own normaliser:
// exp(-beta (d_ij - s_j)) = exp(-beta (d_ij - m_j)) / Z_j is the softmax weight of row i, and s_j <= m_j <= d_ij keeps it <= 1.
// Energies and gradients are accumulated in double from the fp32 inputs and rounded once on the way out.
#include "common.h"
#include "../../include/pepflow_hip.h"
#include "eval_dev.h"

namespace {

constexpr int NT = 256;
constexpr unsigned CL_P = 1, CL_M = 2, CL_C = 4, CL_H = 8;      // peptide, movable (subset of P), context, hot spot (subset of C)
constexpr double CA_CA = 3.8;                                  // ideal distance of consecutive C-alpha atoms
constexpr double D_MIN = 1e-6;                                 // below it a pair gives its energy and no gradient

// maximum over the block (every thread gets it): a maximum does not depend on the order
__device__ __forceinline__ double block_max(double v, double* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = fmax(red[tid], red[tid + h]);
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double dist3(const float* xs, int i, int j, double dx[3]) {
    dx[0] = (double)xs[3 * i] - (double)xs[3 * j];
    dx[1] = (double)xs[3 * i + 1] - (double)xs[3 * j + 1];
    dx[2] = (double)xs[3 * i + 2] - (double)xs[3 * j + 2];
    return sqrt(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2]);
}

__global__ __launch_bounds__(NT) void guidance_kernel(const pf_guidance_args a) {
    __shared__ float xs[PF_GUIDE_MAX_L * 3];
    __shared__ unsigned char cls[PF_GUIDE_MAX_L];
    __shared__ double hs_s[PF_GUIDE_MAX_L], hs_pull[PF_GUIDE_MAX_L];
    __shared__ double red[NT];
    __shared__ int pr_a[PF_GUIDE_MAX_PAIRS], pr_b[PF_GUIDE_MAX_PAIRS];
    __shared__ float pr_lo[PF_GUIDE_MAX_PAIRS], pr_hi[PF_GUIDE_MAX_PAIRS], pr_w[PF_GUIDE_MAX_PAIRS];

    const int b = blockIdx.x, tid = threadIdx.x, L = a.L, B = a.B;
    int s = 0;
    if (a.step) {
        s = *a.step;
        if (s >= a.num_steps) return;                          // (uniform over the grid: the step kernel returns the same way)
    }
    const double t = a.step ? (double)a.ts[s] : (double)a.t[b];
    const float* P = a.params;
    const double w0 = P[0], w1 = P[1], w2 = P[2], w3 = P[3];
    const double r0 = P[4], r1 = P[5], tol = P[7], r3 = P[8], beta = P[9];
    const int min_sep = (int)P[6];
    const double scale = P[10], t_on = P[11], max_shift = P[13];
    const int power = (int)P[12];
    double lam = 0.0;
    if (t >= t_on && t_on < 1.0) {
        const double u = (t - t_on) / (1.0 - t_on);
        lam = scale * (power == 0 ? 1.0 : power == 1 ? u : u * u);
    }
    const size_t row0 = (size_t)b * L;

    // ---- stage positions and row classes ----
    for (int l = tid; l < L; l += NT) {
        const size_t r = row0 + l;
        const bool res = a.res_mask[r] > 0.5f, gen = a.gen_mask[r] > 0.5f;
        const bool fbb = a.res_flags ? (a.res_flags[r] & 1u) != 0 : a.sample_bb != 0;
        unsigned c = 0;
        if (res) {
            if (gen) c = fbb ? (CL_P | CL_M) : CL_P;
            else c = (a.hotspots && a.hotspots[r]) ? (CL_C | CL_H) : CL_C;
        }
        const float* src = (c & CL_M) ? a.pred_trans + r * 3 : a.trans1 + r * 3;
        xs[3 * l] = src[0];
        xs[3 * l + 1] = src[1];
        xs[3 * l + 2] = src[2];
        cls[l] = (unsigned char)c;
    }
    __syncthreads();
    // ---- the sample's restraints: an index outside [0, L) is refused (error[b] = -1, the pair takes no part) ----
    if (tid < PF_GUIDE_MAX_PAIRS) {
        int ia = 0, ib = 0;
        float lo = 0.f, hi = 0.f, w = 0.f;
        if (a.pair_idx) {
            const size_t p = (size_t)b * PF_GUIDE_MAX_PAIRS + tid;
            ia = a.pair_idx[2 * p];
            ib = a.pair_idx[2 * p + 1];
            lo = a.pair_par[3 * p];
            hi = a.pair_par[3 * p + 1];
            w = a.pair_par[3 * p + 2];
        }
        if (!(w > 0.f)) w = 0.f;
        if (w > 0.f && (ia < 0 || ia >= L || ib < 0 || ib >= L)) {
            if (a.error) a.error[b] = -1;
            w = 0.f;
        }
        if (w > 0.f && (cls[ia] == 0 || cls[ib] == 0)) w = 0.f;
        if (w == 0.f) ia = ib = 0;
        pr_a[tid] = ia;
        pr_b[tid] = ib;
        pr_lo[tid] = lo;
        pr_hi[tid] = hi;
        pr_w[tid] = w;
    }
    __syncthreads();

    double e[PF_GUIDE_NTERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // ---- hot spots, pass 1: a thread owns hot spots j; soft-min over the peptide rows with the minimum subtracted ----
    const bool hot = a.hotspots != nullptr && beta > 0.0;
    if (hot) {
        for (int j = tid; j < L; j += NT) {
            if (!(cls[j] & CL_H)) continue;
            double m = 0.0, dx[3];
            int np = 0;
            for (int i = 0; i < L; ++i)
                if (cls[i] & CL_P) {
                    const double d = dist3(xs, i, j, dx);
                    m = (np == 0 || d < m) ? d : m;
                    ++np;
                }
            double sj = 0.0, pull = 0.0;
            if (np > 0) {
                double Z = 0.0;
                for (int i = 0; i < L; ++i)
                    if (cls[i] & CL_P) Z += exp(-beta * (dist3(xs, i, j, dx) - m));
                sj = m - log(Z) / beta;
                pull = fmax(0.0, sj - r3);
            }
            hs_s[j] = sj;
            hs_pull[j] = pull;
            e[3] += pull * pull;
        }
    }
    // ---- restraint energies: thread p owns pair p ----
    if (tid < PF_GUIDE_MAX_PAIRS && pr_w[tid] > 0.f) {
        double dx[3];
        const double d = dist3(xs, pr_a[tid], pr_b[tid], dx);
        const double under = fmax(0.0, (double)pr_lo[tid] - d), over = fmax(0.0, d - (double)pr_hi[tid]);
        e[4] = (double)pr_w[tid] * (under * under + over * over);
    }
    __syncthreads();

    // ---- pass 2: a thread owns rows i ----
    double smax = 0.0;
    for (int i = tid; i < L; i += NT) {
        const unsigned ci = cls[i];
        const size_t r = row0 + i;
        double g[3] = {0.0, 0.0, 0.0};
        if (ci & CL_P) {
            for (int j = 0; j < L; ++j) {
                const unsigned cj = cls[j];
                if (cj == 0 || j == i) continue;
                double dx[3];
                const double d = dist3(xs, i, j, dx);
                double coef = 0.0;                              // dE/dd of this pair
                if (cj & CL_C) {
                    if (d < r0) {
                        const double v = r0 - d;
                        e[0] += v * v;
                        coef -= 2.0 * w0 * v;
                    }
                    if (hot && (cj & CL_H) && hs_pull[j] > 0.0) coef += 2.0 * w3 * hs_pull[j] * exp(-beta * (d - hs_s[j]));
                } else {
                    const int sep = j > i ? j - i : i - j;
                    if (sep >= min_sep && d < r1) {
                        const double v = r1 - d;
                        if (j > i) e[1] += v * v;
                        coef -= 2.0 * w1 * v;
                    }
                    if (sep == 1) {
                        const double dev = fabs(d - CA_CA) - tol;
                        if (dev > 0.0) {
                            if (j > i) e[2] += dev * dev;
                            coef += (d > CA_CA ? 2.0 : -2.0) * w2 * dev;
                        }
                    }
                }
                if (coef != 0.0 && d >= D_MIN) {
                    const double q = coef / d;
                    g[0] += q * dx[0];
                    g[1] += q * dx[1];
                    g[2] += q * dx[2];
                }
            }
        }
        if (ci & CL_M) {
            for (int p = 0; p < PF_GUIDE_MAX_PAIRS; ++p) {
                if (!(pr_w[p] > 0.f)) continue;
                const int ia = pr_a[p], ib = pr_b[p];
                if ((ia != i && ib != i) || ia == ib) continue;
                double dx[3];
                const double d = dist3(xs, i, ia == i ? ib : ia, dx);
                const double coef = (double)pr_w[p] * (2.0 * fmax(0.0, d - (double)pr_hi[p]) - 2.0 * fmax(0.0, (double)pr_lo[p] - d));
                if (coef != 0.0 && d >= D_MIN) {
                    const double q = coef / d;
                    g[0] += q * dx[0];
                    g[1] += q * dx[1];
                    g[2] += q * dx[2];
                }
            }
        } else {
            g[0] = g[1] = g[2] = 0.0;
        }
        if (a.grad) {
            a.grad[r * 3] = (float)g[0];
            a.grad[r * 3 + 1] = (float)g[1];
            a.grad[r * 3 + 2] = (float)g[2];
        }
        if (a.guided_trans) {
            const double sh[3] = {lam * g[0], lam * g[1], lam * g[2]};
            const double n = sqrt(sh[0] * sh[0] + sh[1] * sh[1] + sh[2] * sh[2]);
            if ((ci & CL_M) && n > 0.0) {
                const double f = fmin(1.0, max_shift / fmax(n, 1e-12));
                a.guided_trans[r * 3] = (float)((double)xs[3 * i] - sh[0] * f);
                a.guided_trans[r * 3 + 1] = (float)((double)xs[3 * i + 1] - sh[1] * f);
                a.guided_trans[r * 3 + 2] = (float)((double)xs[3 * i + 2] - sh[2] * f);
                smax = fmax(smax, n * f);
            } else {                                            // the prediction's bits
                const uint32_t* src = reinterpret_cast<const uint32_t*>(a.pred_trans) + r * 3;
                uint32_t* dst = reinterpret_cast<uint32_t*>(a.guided_trans) + r * 3;
                dst[0] = src[0];
                dst[1] = src[1];
                dst[2] = src[2];
            }
        }
    }
    const double wts[PF_GUIDE_NTERMS] = {w0, w1, w2, w3, 1.0};
    float* eout = a.energy + ((size_t)s * B + b) * PF_GUIDE_NTERMS;
#pragma unroll
    for (int k = 0; k < PF_GUIDE_NTERMS; ++k) {
        const double tot = block_sum<NT>(e[k], red, tid);
        if (tid == 0) eout[k] = (float)(wts[k] * tot);
    }
    if (a.shift_max) {
        const double m = block_max(smax, red, tid);
        if (tid == 0) a.shift_max[(size_t)s * B + b] = (float)m;
    }
}

}  // namespace

extern "C" int pf_guidance_fwd(const pf_guidance_args* a, pf_stream_t stream) {
    if (!a || !a->pred_trans || !a->trans1 || !a->gen_mask || !a->res_mask || !a->params || !a->energy || a->B <= 0 || a->L <= 0)
        return PF_E_BADARG;
    if ((a->pair_idx == nullptr) != (a->pair_par == nullptr)) return PF_E_BADARG;
    if (a->step) {
        if (!a->ts || a->num_steps <= 0 || !a->guided_trans || !a->shift_max) return PF_E_BADARG;
    } else if (!a->t) {
        return PF_E_BADARG;
    }
    if (a->L > PF_GUIDE_MAX_L) return PF_E_TOOLARGE;
    hipLaunchKernelGGL(guidance_kernel, dim3((unsigned)a->B), dim3(NT), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
