// pf_superpose_fwd / pf_binding_site_fwd -- evaluation of sampled peptides: superposition RMSD (Kabsch, and the reflection-allowed
// rotation of pepflow/modules/common/geometry.py:18-56 align / batch_align), sequence identity, and the binding-site contacts of
// eval/geometry.py:93-110.
//
// Superposition: one wave per pair of a work list, four pairs per 256-thread block.  The lanes stride over the points; the sums
// are all-reduced in fp64 with an xor butterfly, after which every lane holds bit-identical sums and runs the 3x3 eigen-work
// redundantly (no broadcast, uniform control flow).  Pass 1: count, centroids, plain squared deviation, identity.  Pass 2: the
// centred cross terms S = X^T Y and the squared norms E_x, E_y.  Pass 3 (optional): the aligned coordinates of all points.
#include "common.h"
#include "../../include/pepflow_hip.h"
#include "superpose_dev.h"

namespace {

__global__ __launch_bounds__(256) void superpose_kernel(pf_superpose_args a) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.P) return;                                          // whole waves only: no block barrier below
    const int i = a.pairs[2 * p], j = a.pairs[2 * p + 1];
    const bool valid = i >= 0 && i < a.Bx && j >= 0 && j < a.By;
    const int N = a.N;
    const float* X = a.x + (size_t)(valid ? i : 0) * N * 3;
    const float* Y = a.y + (size_t)(valid ? j : 0) * N * 3;
    const unsigned char* MX = a.mx + (size_t)(valid ? i : 0) * N;
    const unsigned char* MY = a.my + (size_t)(valid ? j : 0) * N;
    const bool with_aa = a.ident != nullptr;
    const int64_t* AX = with_aa ? a.aa_x + (size_t)(valid ? i : 0) * N : nullptr;
    const int64_t* AY = with_aa ? a.aa_y + (size_t)(valid ? j : 0) * N : nullptr;

    // pass 1: count, centroids, plain squared deviation, identical residue types
    double n = 0.0, sx[3] = {0.0, 0.0, 0.0}, sy[3] = {0.0, 0.0, 0.0}, dev = 0.0, same = 0.0;
    if (valid)
        for (int k = lane; k < N; k += 64) {
            if (!(MX[k] && MY[k])) continue;
            n += 1.0;
            double d2 = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double xv = X[(size_t)k * 3 + c], yv = Y[(size_t)k * 3 + c];
                sx[c] += xv;
                sy[c] += yv;
                d2 += (xv - yv) * (xv - yv);
            }
            dev += d2;
            if (with_aa && AX[k] == AY[k]) same += 1.0;
        }
    n = wave_sum_f64(n);
    dev = wave_sum_f64(dev);
    if (with_aa) same = wave_sum_f64(same);
#pragma unroll
    for (int c = 0; c < 3; ++c) { sx[c] = wave_sum_f64(sx[c]); sy[c] = wave_sum_f64(sy[c]); }

    const float qnan = __int_as_float(0x7fc00000);
    if (n == 0.0) {
        if (lane == 0) {
            a.rmsd_plain[p] = qnan;
            a.rmsd[p] = qnan;
            a.count[p] = 0;
            if (a.ident) a.ident[p] = qnan;
            if (a.degenerate) a.degenerate[p] = 1;
            if (a.rot)
                for (int k = 0; k < 9; ++k) a.rot[(size_t)p * 9 + k] = (k % 4 == 0) ? 1.f : 0.f;
            if (a.trans)
                for (int k = 0; k < 3; ++k) a.trans[(size_t)p * 3 + k] = qnan;
        }
        if (a.aligned)
            for (int k = lane; k < N * 3; k += 64) a.aligned[(size_t)p * N * 3 + k] = qnan;
        return;
    }
    double mx[3], my[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { mx[c] = sx[c] / n; my[c] = sy[c] / n; }

    // pass 2: centred cross terms and squared norms
    double S[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, ex = 0.0, ey = 0.0;
    for (int k = lane; k < N; k += 64) {
        if (!(MX[k] && MY[k])) continue;
        double xc[3], yc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xc[c] = (double)X[(size_t)k * 3 + c] - mx[c];
            yc[c] = (double)Y[(size_t)k * 3 + c] - my[c];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            ex += xc[r] * xc[r];
            ey += yc[r] * yc[r];
#pragma unroll
            for (int c = 0; c < 3; ++c) S[r][c] += xc[r] * yc[c];
        }
    }
    ex = wave_sum_f64(ex);
    ey = wave_sum_f64(ey);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) S[r][c] = wave_sum_f64(S[r][c]);

    double R[3][3], lam;
    const bool degenerate = kabsch_rotation(S, a.allow_reflection != 0, R, lam);
    double t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = my[r] - (R[r][0] * mx[0] + R[r][1] * mx[1] + R[r][2] * mx[2]);

    if (lane == 0) {
        const double e = ex + ey - 2.0 * lam;
        a.rmsd_plain[p] = (float)sqrt(dev / n);
        a.rmsd[p] = (float)sqrt((e > 0.0 ? e : 0.0) / n);
        a.count[p] = (int)n;
        if (a.ident) a.ident[p] = (float)(same / n);
        if (a.degenerate) a.degenerate[p] = degenerate ? 1 : 0;
        if (a.rot)
#pragma unroll
            for (int k = 0; k < 9; ++k) a.rot[(size_t)p * 9 + k] = (float)R[k / 3][k % 3];
        if (a.trans)
#pragma unroll
            for (int k = 0; k < 3; ++k) a.trans[(size_t)p * 3 + k] = (float)t[k];
    }
    // pass 3: the transform applied to every point of x[i], masked ones included (the reference's output)
    if (a.aligned)
        for (int k = lane; k < N; k += 64) {
            const double xv[3] = {X[(size_t)k * 3], X[(size_t)k * 3 + 1], X[(size_t)k * 3 + 2]};
#pragma unroll
            for (int r = 0; r < 3; ++r)
                a.aligned[((size_t)p * N + k) * 3 + r] = (float)(R[r][0] * xv[0] + R[r][1] * xv[1] + R[r][2] * xv[2] + t[r]);
        }
}

// binding-site contacts: one block per sample, a thread per context residue; the peptide CAs go through LDS in chunks of 256
__global__ __launch_bounds__(256) void binding_site_kernel(pf_binding_site_args a) {
    __shared__ float ps[256][3], pn[256][3];
    __shared__ unsigned char pg[256];
    __shared__ int n_both, n_native;
    const int b = blockIdx.x, L = a.L;
    if (threadIdx.x == 0) { n_both = 0; n_native = 0; }
    const double cut2 = (double)a.cutoff * (double)a.cutoff;
    int both = 0, nat = 0;
    for (int r0 = 0; r0 < L; r0 += 256) {
        const int r = r0 + threadIdx.x;
        const size_t br = (size_t)b * L + r;
        bool ctx = false;
        double c[3] = {0.0, 0.0, 0.0};
        if (r < L) {
            const size_t ca = br * a.n_atoms + a.ca_atom;
            ctx = a.res_mask[br] && !a.gen_mask[br] && a.ctx_atom_mask[ca];
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = a.ctx_pos[ca * 3 + k];
        }
        bool hit_s = false, hit_n = false;
        for (int q0 = 0; q0 < L; q0 += 256) {
            __syncthreads();
            const int q = q0 + threadIdx.x;
            if (q < L) {
                const size_t bq = (size_t)b * L + q;
                pg[threadIdx.x] = a.gen_mask[bq] && a.res_mask[bq];
#pragma unroll
                for (int k = 0; k < 3; ++k) { ps[threadIdx.x][k] = a.pep_sample[bq * 3 + k]; pn[threadIdx.x][k] = a.pep_native[bq * 3 + k]; }
            }
            __syncthreads();
            const int m = L - q0 < 256 ? L - q0 : 256;
            if (ctx)
                for (int u = 0; u < m; ++u) {
                    if (!pg[u]) continue;
                    double ds = 0.0, dn = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double es = c[k] - ps[u][k], en = c[k] - pn[u][k];
                        ds += es * es;
                        dn += en * en;
                    }
                    hit_s |= ds <= cut2;
                    hit_n |= dn <= cut2;
                }
        }
        if (r < L) {
            a.site_sample[br] = hit_s ? 1 : 0;
            a.site_native[br] = hit_n ? 1 : 0;
        }
        both += hit_s && hit_n;
        nat += hit_n;
    }
    __syncthreads();
    atomicAdd(&n_both, both);
    atomicAdd(&n_native, nat);
    __syncthreads();
    if (threadIdx.x == 0) a.bsr[b] = (float)((double)n_both / ((double)n_native + 1e-10));
}

}  // namespace

extern "C" int pf_superpose_fwd(const pf_superpose_args* a, pf_stream_t stream) {
    if (!a || !a->x || !a->y || !a->mx || !a->my || !a->pairs || !a->rmsd_plain || !a->rmsd || !a->count || a->Bx <= 0 || a->By <= 0 ||
        a->N <= 0 || a->P < 0 || (!a->rot != !a->trans) || (a->ident && (!a->aa_x || !a->aa_y)))
        return PF_E_BADARG;
    if ((long long)a->N * 3 > 0x7fffffffLL) return PF_E_TOOLARGE;
    if (a->P == 0) return 0;
    hipLaunchKernelGGL(superpose_kernel, dim3((unsigned)((a->P + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}

extern "C" int pf_binding_site_fwd(const pf_binding_site_args* a, pf_stream_t stream) {
    if (!a || !a->ctx_pos || !a->ctx_atom_mask || !a->res_mask || !a->gen_mask || !a->pep_sample || !a->pep_native || !a->site_sample ||
        !a->site_native || !a->bsr || a->B <= 0 || a->L <= 0 || a->n_atoms <= 0 || a->ca_atom < 0 || a->ca_atom >= a->n_atoms ||
        !(a->cutoff >= 0.f))
        return PF_E_BADARG;
    hipLaunchKernelGGL(binding_site_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
