// Steered sampling: particle resampling by guidance energy after one sampler step (pf_sampler_steer; formulas and conventions:
// include/pepflow_hip.h).  The reference has no such call.
//
// Two launches per step, after pf_sampler_step* has taken the Euler step and bumped the counter (so s = step[0] - 1):
//   decide  one workgroup of 256 threads per particle group: the log-weights take the difference potential of the energies
//           pf_guidance_fwd recorded for step s, and at a resampling moment with a low effective sample size the group is resampled
//           systematically; the kernel writes which slot every slot continues from (ancestors) and the records;
//   gather  one thread per row: a slot whose ancestor is another slot copies that slot's rows of the seven state tensors.
// Parameters, group structure, number of groups and the uniforms are read from device memory: a captured graph serves later calls that
// rewrite them.  All arithmetic of the decision is double, every sum runs in ascending member order on one thread, there is no atomic:
// two runs give the same bits, and a float64 restatement in the same order differs at most in the last bits of exp().
#include "common.h"
#include "flow_dev.h"
#include "../../include/pepflow_hip.h"

namespace {

constexpr int NT = 256;
constexpr int MAXG = PF_STEER_MAX_GROUP;

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

__global__ __launch_bounds__(NT) void steer_decide_kernel(const pf_sampler_steer_args a) {
    __shared__ double w[MAXG];          // log-weight of member i, then exp(logw_i - M)
    __shared__ double csum[MAXG];       // raw running sum C_i
    __shared__ double ep[MAXG];         // eprev of member i after the update
    __shared__ int mem[MAXG];           // sample index of member i
    __shared__ int ak[MAXG];            // a_k, then the local ancestor of slot i
    __shared__ int cnt[MAXG];           // c_i
    __shared__ double red[NT];
    __shared__ double sh_S, sh_Q;
    __shared__ int sh_last;

    const int g = blockIdx.x, tid = threadIdx.x;
    const bool alone = a.step == nullptr;
    const int s = alone ? 0 : a.step[0] - 1;
    if (!alone && (s < 0 || s >= a.num_steps)) return;         // (uniform over the grid)
    if (g >= a.n_groups[0]) return;
    const int B = a.B;
    const int lo = a.group_ptr[g], hi = a.group_ptr[g + 1];
    const int n = hi - lo;
    if (lo < 0 || hi > B || n <= 0 || n > MAXG) return;         // (the host refuses such a structure; nothing is read through it)
    int bad = 0;
    for (int i = tid; i < n; i += NT) {
        const int m = a.members[lo + i];
        mem[i] = m;
        bad |= (m < 0 || m >= B);
    }
    if (__syncthreads_or(bad)) return;

    const double lam = a.params[0], ess_frac = a.params[2], t_on = a.params[3], t_off = a.params[4];
    int every = (int)a.params[1];
    if (every < 1) every = 1;
    bool active = true, moment = true;
    if (!alone) {
        const double t = (double)a.ts[s];
        active = t_on <= t && t <= t_off;
        moment = active && s < a.num_steps - 1 && (s + 1) % every == 0;
    }
    const size_t rec = (size_t)s * (size_t)B;                   // (s = 0 when alone)
    const double NEG_INF = -HUGE_VAL;

    // ---- the difference potential: logw += -lam (E - eprev), eprev = E ----
    double mx = NEG_INF;
    for (int i = tid; i < n; i += NT) {
        const int m = mem[i];
        const float* e = a.energy + (rec + (size_t)m) * 5;
        const double E = (((double)e[0] + (double)e[1]) + (double)e[2] + (double)e[3]) + (double)e[4];
        double lw = a.logw[m];
        double pv = a.eprev ? a.eprev[m] : 0.0;
        if (active) {
            if (!finite_d(E)) lw = NEG_INF;
            else { lw = lw + (-lam) * (E - pv); pv = E; }
        }
        if (lw != lw) lw = NEG_INF;
        if (active) {
            a.logw[m] = lw;
            if (a.eprev) a.eprev[m] = pv;
        }
        if (a.logw_rec) a.logw_rec[rec + m] = lw;
        w[i] = lw;
        ep[i] = pv;
        mx = lw > mx ? lw : mx;
    }
    // the maximum: independent of the order it is taken in
    red[tid] = mx;
    __syncthreads();
    for (int h = NT / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] = red[tid + h] > red[tid] ? red[tid + h] : red[tid];
        __syncthreads();
    }
    const double M = red[0];
    const bool ok = finite_d(M);

    // ---- effective sample size: S and Q summed by ONE thread in ascending member order ----
    double ess = 0.0;
    if (ok) {
        for (int i = tid; i < n; i += NT) w[i] = exp(w[i] - M);
        __syncthreads();
        if (tid == 0) {
            double S = 0.0, Q = 0.0;
            int last = 0;
            for (int i = 0; i < n; ++i) {
                const double wi = w[i];
                S = S + wi;
                Q = Q + wi * wi;
                csum[i] = S;
                if (wi > 0.0) last = i;
            }
            sh_S = S; sh_Q = Q; sh_last = last;
        }
        __syncthreads();
        ess = sh_S * sh_S / sh_Q;
    }
    const bool resample = moment && ok && (ess_frac >= 1.0 || ess <= ess_frac * (double)n);
    if (tid == 0) {
        a.ess[rec + g] = ess;
        a.code[rec + g] = !moment ? 0 : !ok ? -1 : resample ? 2 : 1;
    }
    if (!resample) {
        for (int i = tid; i < n; i += NT) a.ancestors[rec + mem[i]] = mem[i];
        return;
    }

    // ---- systematic resampling: one uniform per (step, group) ----
    double u;
    if (a.u) u = a.u[rec + g];
    else {
        const int m0 = mem[0];
        const uint64_t seed = a.seed_dev ? a.seed_dev[0] : a.seed;
        const long long gs = a.sample_ids ? (long long)a.sample_ids[m0] : (a.seed_dev ? (long long)a.seed_dev[1] : (long long)a.first_sample) + m0;
        uint32_t c[4] = {0u, 0xC0000000u | (uint32_t)s, (uint32_t)gs, (uint32_t)((uint64_t)gs >> 32)};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        u = ((double)(c[0] >> 8) + 0.5) * 5.9604644775390625e-08;
    }
    const double S = sh_S;
    const int last = sh_last;
    for (int k = tid; k < n; k += NT) {
        const double thr = ((u + (double)k) / (double)n) * S;
        int l = 0, r = n;                                       // first i with C_i > thr
        while (l < r) {
            const int mid = (l + r) >> 1;
            if (csum[mid] > thr) r = mid; else l = mid + 1;
        }
        ak[k] = l < n ? l : last;                               // rounding left none: the last slot with a positive weight
    }
    __syncthreads();
    // c_i: a_k ascends in k, so the k with a_k = i form one run
    for (int i = tid; i < n; i += NT) {
        int l = 0, r = n;
        while (l < r) { const int mid = (l + r) >> 1; if (ak[mid] >= i) r = mid; else l = mid + 1; }
        const int first = l;
        r = n;
        while (l < r) { const int mid = (l + r) >> 1; if (ak[mid] > i) r = mid; else l = mid + 1; }
        cnt[i] = l - first;
    }
    __syncthreads();
    // stable assignment: a slot with c_i >= 1 keeps its particle; the dead slots in ascending order take "i repeated c_i - 1 times"
    for (int i = tid; i < n; i += NT) ak[i] = i;
    __syncthreads();
    if (tid == 0) {
        int j = 0;
        for (int i = 0; i < n; ++i)
            for (int r = 1; r < cnt[i]; ++r) {
                while (j < n && cnt[j] != 0) ++j;
                if (j < n) ak[j++] = i;
            }
    }
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
        const int m = mem[i], src = ak[i];
        a.ancestors[rec + m] = mem[src];
        a.logw[m] = 0.0;
        if (a.eprev && src != i) a.eprev[m] = ep[src];          // (a source is a surviving slot: nobody writes its eprev here)
    }
}

// In place, no second buffer and no third launch: the decide kernel's stable assignment makes every source a SURVIVING slot
// (ancestors[src] == src) and every destination a dead one, so the rows read here are rows no thread of this launch writes.
__global__ __launch_bounds__(NT) void steer_gather_kernel(const pf_sampler_steer_args a) {
    const int row = blockIdx.x * NT + threadIdx.x;
    const int n = a.B * a.L;
    if (row >= n) return;
    const bool alone = a.step == nullptr;
    const int s = alone ? 0 : a.step[0] - 1;
    if (!alone && (s < 0 || s >= a.num_steps - 1)) return;      // (the last step never gathers)
    const int b = row / a.L, l = row - b * a.L;
    const int anc = a.ancestors[(size_t)s * a.B + b];
    if (anc == b || anc < 0 || anc >= a.B) return;
    const size_t d = (size_t)row, r = (size_t)anc * a.L + l;
    // raw bits
    uint32_t* rot = (uint32_t*)a.rot_t; uint32_t* tr = (uint32_t*)a.trans_t; uint32_t* ang = (uint32_t*)a.ang_t;
    uint32_t* sx = (uint32_t*)a.simplex_t; uint32_t* t0 = (uint32_t*)a.trans0; uint32_t* s0 = (uint32_t*)a.simplex0;
#pragma unroll
    for (int k = 0; k < 9; ++k) rot[d * 9 + k] = rot[r * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { tr[d * 3 + k] = tr[r * 3 + k]; t0[d * 3 + k] = t0[r * 3 + k]; }
#pragma unroll
    for (int k = 0; k < 5; ++k) ang[d * 5 + k] = ang[r * 5 + k];
    a.seq_t[d] = a.seq_t[r];
#pragma unroll
    for (int k = 0; k < KCLS; ++k) { sx[d * KCLS + k] = sx[r * KCLS + k]; s0[d * KCLS + k] = s0[r * KCLS + k]; }
}

}  // namespace

extern "C" int pf_sampler_steer(const pf_sampler_steer_args* a, pf_stream_t stream) {
    if (!a || !a->params || !a->group_ptr || !a->members || !a->n_groups || !a->energy) return PF_E_BADARG;
    if (a->B <= 0 || a->L <= 0 || a->num_steps <= 0 || a->max_group <= 0) return PF_E_BADARG;
    if (!a->logw || !a->ancestors || !a->ess || !a->code) return PF_E_BADARG;
    if (a->step && (!a->ts || !a->eprev || !a->logw_rec)) return PF_E_BADARG;          // sampler mode: the grid, eprev and every record
    const int n_state = (a->rot_t != nullptr) + (a->trans_t != nullptr) + (a->ang_t != nullptr) + (a->seq_t != nullptr) +
                        (a->simplex_t != nullptr) + (a->trans0 != nullptr) + (a->simplex0 != nullptr);
    if (n_state != 0 && n_state != 7) return PF_E_BADARG;                              // all seven state tensors or none
    if (a->max_group > PF_STEER_MAX_GROUP) return PF_E_TOOLARGE;
    hipLaunchKernelGGL(steer_decide_kernel, dim3((unsigned)a->B), dim3(NT), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    if (n_state == 7) {
        const long long n = (long long)a->B * a->L;
        if (n > 0x7fffffffLL) return PF_E_TOOLARGE;
        hipLaunchKernelGGL(steer_gather_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, *a);
        PF_CHECK_LAUNCH();
    }
    return 0;
}
