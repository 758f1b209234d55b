// pf_optim_step -- the optimizer block of a training iteration (train.py:135-146 / train_ddp.py:144-155 of the reference: zero the NaN
// gradient entries, clip_grad_norm_, torch.optim.Adam / AdamW step) over ALL parameter tensors in three launches, without a host read.
// Written from the formulas of Kingma & Ba (Adam), Loshchilov & Hutter (AdamW) and the documented behaviour of clip_grad_norm_;
// tests/optim_oracle.py restates them in float64 and is pinned to torch's CPU optimizers.
//
// Conventions (include/pepflow_hip.h has them in full):
//   tables    everything that describes a step lives in DEVICE memory: the tensor table (pf_optim_tensor), the hyper-parameter rows
//             (double), the chunk list (tensor, first element), the step counters.  A captured launch stays valid when lr changes.
//   chunk     PF_OPTIM_CHUNK elements of ONE tensor, one workgroup of 256 threads; thread i owns the quads i, i + 256, ... of the chunk
//             in BOTH the 16-byte and the 4-byte path, so a tensor's results do not depend on its alignment.
//   phase 1   optim_norm_kernel: per chunk the sum of g^2 in float64 with NaN entries as 0, the NaN count, an inf flag -> workspace.
//   phase 1b  optim_reduce_kernel (one workgroup): the partials in a fixed order -> total_norm, the clip coefficient, the skip flag,
//             the result block; it then advances the step counter of every active tensor (one thread per tensor: no race between
//             the chunks of a tensor, which only READ it in phase 2).
//   phase 2   optim_update_kernel: the Adam / AdamW update of a chunk with the clip applied in registers.  Gradients are never written.
// No atomics; every word has one writer and every sum one order: bit-identical from run to run.  The only coupling between tensors
// is the clip coefficient (and the inf guard), which is a function of the total norm.
#include <limits.h>
#include <math.h>
#include "common.h"
#include "../../include/pepflow_hip.h"

namespace {

constexpr int NT = 256;
constexpr int QUADS = PF_OPTIM_CHUNK / 4;                 // float4 groups of a chunk
constexpr int QPT = QUADS / NT;                           // ... per thread
constexpr int HEADER = 64;                                // workspace: header | double partial[n] | int nan[n] | int inf[n]
static_assert(PF_OPTIM_CHUNK % (4 * NT) == 0, "a chunk is a whole number of quads per thread");
static_assert(sizeof(pf_optim_tensor) == 48, "the host builds this table as a 48-byte record");

struct WorkHeader { double coef; int skip; };

__device__ __forceinline__ double* work_partial(void* work) { return reinterpret_cast<double*>(static_cast<char*>(work) + HEADER); }
__device__ __forceinline__ int* work_nan(void* work, int n_chunks) { return reinterpret_cast<int*>(work_partial(work) + n_chunks); }
__device__ __forceinline__ int* work_inf(void* work, int n_chunks) { return work_nan(work, n_chunks) + n_chunks; }

// the chunk's tensor and range; false (nothing to do) for an entry that does not describe an active slice
struct Slice { pf_optim_tensor t; int first, n; };
__device__ __forceinline__ bool chunk_slice(const pf_optim_args& a, int c, Slice& s) {
    const int ti = a.chunks[2 * c];
    s.first = a.chunks[2 * c + 1];
    if (ti < 0 || ti >= a.n_tensors || s.first < 0) return false;
    s.t = a.tensors[ti];
    const long long left = (long long)s.t.numel - s.first;
    s.n = left < PF_OPTIM_CHUNK ? (int)left : PF_OPTIM_CHUNK;
    return s.t.active != 0 && s.n > 0 && s.t.group >= 0 && s.t.group < a.n_groups && s.t.param && s.t.grad;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// up to four consecutive floats from p: one 16-byte load where VEC and the quad is whole, scalar loads otherwise
template <bool VEC>
__device__ __forceinline__ void load_quad(const float* __restrict__ p, int cnt, float (&v)[4]) {
    if (VEC && cnt == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < cnt ? p[e] : 0.f;
    }
}
template <bool VEC>
__device__ __forceinline__ void store_quad(float* __restrict__ p, int cnt, const float (&v)[4]) {
    if (VEC && cnt == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < cnt) p[e] = v[e];
    }
}

template <bool VEC>
__device__ __forceinline__ void norm_slice(const float* __restrict__ g, int n, double& sum, int& nans, int& infs) {
    float v[QPT][4];
    int cnt[QPT];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {                        // every load of the thread in flight before the first use
        const int q = (int)threadIdx.x + NT * j;
        const int left = n - 4 * q;
        cnt[j] = left < 0 ? 0 : left > 4 ? 4 : left;
        load_quad<VEC>(g + 4 * (cnt[j] ? q : 0), cnt[j], v[j]);
    }
#pragma unroll
    for (int j = 0; j < QPT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= cnt[j]) continue;
            const float x = v[j][e];
            if (isnan(x)) { ++nans; continue; }
            infs |= isinf(x) ? 1 : 0;
            sum += (double)x * (double)x;
        }
}

__global__ __launch_bounds__(NT) void optim_norm_kernel(pf_optim_args a) {
    const int c = blockIdx.x;
    Slice s;
    double sum = 0.0;
    int nans = 0, infs = 0;
    if (chunk_slice(a, c, s)) {                            // uniform over the workgroup
        const float* g = s.t.grad + s.first;
        if (aligned16(s.t.param) && aligned16(s.t.grad) && aligned16(a.exp_avg + s.t.exp_avg_off) && aligned16(a.exp_avg_sq + s.t.exp_avg_sq_off))
            norm_slice<true>(g, s.n, sum, nans, infs);
        else
            norm_slice<false>(g, s.n, sum, nans, infs);
    }
    // fixed tree inside a wave, then the four waves in order
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sum += __shfl_xor(sum, m);
        nans += __shfl_xor(nans, m);
        infs |= __shfl_xor(infs, m);
    }
    __shared__ double s_sum[NT / 64];
    __shared__ int s_nan[NT / 64], s_inf[NT / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_sum[wave] = sum; s_nan[wave] = nans; s_inf[wave] = infs; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s_sum[0];
        int n = s_nan[0], f = s_inf[0];
        for (int w = 1; w < NT / 64; ++w) { t += s_sum[w]; n += s_nan[w]; f |= s_inf[w]; }
        work_partial(a.work)[c] = t;
        work_nan(a.work, a.n_chunks)[c] = n;
        work_inf(a.work, a.n_chunks)[c] = f;
    }
}

__global__ __launch_bounds__(NT) void optim_reduce_kernel(pf_optim_args a) {
    __shared__ double s_sum[NT];
    __shared__ int s_nan[NT], s_inf[NT], s_skip;
    const int tid = threadIdx.x;
    const double* partial = work_partial(a.work);
    const int* pn = work_nan(a.work, a.n_chunks);
    const int* pi = work_inf(a.work, a.n_chunks);
    double sum = 0.0;
    int nans = 0, infs = 0;
    for (int c = tid; c < a.n_chunks; c += NT) { sum += partial[c]; nans += pn[c]; infs |= pi[c]; }
    s_sum[tid] = sum; s_nan[tid] = nans; s_inf[tid] = infs;
    __syncthreads();
    for (int h = NT / 2; h >= 1; h >>= 1) {
        if (tid < h) { s_sum[tid] += s_sum[tid + h]; s_nan[tid] += s_nan[tid + h]; s_inf[tid] |= s_inf[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double total = sqrt(s_sum[0]);
        const int skip = (s_inf[0] != 0 || !isfinite(total)) ? 1 : 0;
        const double max_norm = a.hyper[0];
        double coef = 1.0;
        if (max_norm > 0.0) {                              // (false for NaN: no clipping)
            coef = max_norm / (total + 1e-6);
            if (!(coef < 1.0)) coef = 1.0;
        }
        WorkHeader* h = reinterpret_cast<WorkHeader*>(a.work);
        h->coef = coef;
        h->skip = skip;
        reinterpret_cast<float*>(a.result)[0] = skip ? INFINITY : (float)total;
        a.result[1] = s_nan[0];
        a.result[2] += skip;
        s_skip = skip;
    }
    __syncthreads();
    if (s_skip) return;
    for (int t = tid; t < a.n_tensors; t += NT)
        if (a.tensors[t].active) a.steps[t] += 1;
}

// the scalars of a tensor's update: float64, as the host wrote them; the two that enter the fp32 quotient rounded once
struct Scalars { double coef, b1, w1, b2, w2, wd, decay, step_size; float eps, bc2_sqrt; int l2; };

template <bool VEC>
__device__ __forceinline__ void update_slice(const Slice& s, float* __restrict__ m, float* __restrict__ v, const Scalars& k) {
    float* __restrict__ p = s.t.param + s.first;
    const float* __restrict__ g = s.t.grad + s.first;
    float P[QPT][4], G[QPT][4], M[QPT][4], V[QPT][4];
    int cnt[QPT], off[QPT];
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        const int q = (int)threadIdx.x + NT * j;
        const int left = s.n - 4 * q;
        cnt[j] = left < 0 ? 0 : left > 4 ? 4 : left;
        off[j] = 4 * (cnt[j] ? q : 0);
        load_quad<VEC>(p + off[j], cnt[j], P[j]);
        load_quad<VEC>(g + off[j], cnt[j], G[j]);
        load_quad<VEC>(m + off[j], cnt[j], M[j]);
        load_quad<VEC>(v + off[j], cnt[j], V[j]);
    }
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
        if (cnt[j] == 0) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // the moments and the final subtraction in float64 (a handful of full-rate FMAs per element of a memory-bound pass),
            // each stored value rounded ONCE; the quotient m / (sqrt(v) / sqrt(bc2) + eps) in fp32 from the rounded moments
            double x = (double)P[j][e];
            const float g32 = G[j][e];
            double gr = k.coef * (double)(isnan(g32) ? 0.f : g32);
            if (k.l2) gr = fma(k.wd, x, gr);               // Adam: g += wd p
            x *= k.decay;                                  // AdamW: p *= 1 - lr wd (1 otherwise)
            const float mn = (float)fma(k.b1, (double)M[j][e], k.w1 * gr);
            const float vn = (float)fma(k.b2, (double)V[j][e], (k.w2 * gr) * gr);
            const float denom = sqrtf(vn) / k.bc2_sqrt + k.eps;
            P[j][e] = (float)fma(-k.step_size, (double)(mn / denom), x);
            M[j][e] = mn;
            V[j][e] = vn;
        }
        store_quad<VEC>(p + off[j], cnt[j], P[j]);
        store_quad<VEC>(m + off[j], cnt[j], M[j]);
        store_quad<VEC>(v + off[j], cnt[j], V[j]);
    }
}

__global__ __launch_bounds__(NT) void optim_update_kernel(pf_optim_args a) {
    const WorkHeader* h = reinterpret_cast<const WorkHeader*>(a.work);
    if (h->skip) return;
    Slice s;
    if (!chunk_slice(a, blockIdx.x, s)) return;           // uniform over the workgroup
    const int ti = a.chunks[2 * blockIdx.x];
    __shared__ Scalars sk;
    if (threadIdx.x == 0) {
        // bias corrections in float64: an fp32 1 - 0.999^t carries a relative error near 6e-5 at t = 1
        const double* r = a.hyper + 8 * (1 + s.t.group);
        const double lr = r[0], b1 = r[1], b2 = r[2], eps = r[3], wd = r[4];
        const double t = (double)a.steps[ti];              // already advanced by optim_reduce_kernel: t = step + 1
        const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
        Scalars k;
        k.coef = h->coef;
        k.b1 = b1; k.w1 = 1.0 - b1;
        k.b2 = b2; k.w2 = 1.0 - b2;
        k.eps = (float)eps;
        k.l2 = (r[5] == 0.0 && wd != 0.0) ? 1 : 0;
        k.wd = wd;
        k.decay = r[5] != 0.0 ? 1.0 - lr * wd : 1.0;
        k.step_size = lr / bc1;
        k.bc2_sqrt = (float)sqrt(bc2);
        sk = k;
    }
    __syncthreads();
    const Scalars k = sk;
    float* m = a.exp_avg + s.t.exp_avg_off + s.first;
    float* v = a.exp_avg_sq + s.t.exp_avg_sq_off + s.first;
    if (aligned16(s.t.param) && aligned16(s.t.grad) && aligned16(a.exp_avg + s.t.exp_avg_off) && aligned16(a.exp_avg_sq + s.t.exp_avg_sq_off))
        update_slice<true>(s, m, v, k);
    else
        update_slice<false>(s, m, v, k);
}

}  // namespace

extern "C" int pf_optim_work_bytes(int n_chunks) {
    if (n_chunks < 1 || n_chunks > (INT_MAX - HEADER) / 16) return -1;
    return HEADER + 16 * n_chunks;
}

extern "C" int pf_optim_step(const pf_optim_args* a, pf_stream_t stream) {
    if (!a || !a->tensors || !a->hyper || !a->chunks || !a->exp_avg || !a->exp_avg_sq || !a->steps || !a->work || !a->result ||
        a->n_tensors < 1 || a->n_groups < 1 || pf_optim_work_bytes(a->n_chunks) < 0)
        return PF_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)a->n_chunks), dim3(NT), 0, s, *a);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(optim_reduce_kernel, dim3(1), dim3(NT), 0, s, *a);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(optim_update_kernel, dim3((unsigned)a->n_chunks), dim3(NT), 0, s, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
