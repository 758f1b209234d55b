// Device-resident flow-matching sampler updates (models_con/flow_model.py:229-374) and the
// manifold maps they use: SO(3) log/exp/geodesic (data/so3_utils.py:88-311,486-520), torus
// geodesic (models_con/torus.py:5-26), simplex Euler step + categorical draws
// (pepflow/modules/common/layers.py:10-22), torsion masking (models_con/torsion.py:230-232).
// One thread per residue; everything per-residue is fused into one launch per step.
#include "common.h"
#include "flow_dev.h"
#include "../../include/pepflow_hip.h"

namespace {


// ---- conditioned sampling (pf_sampler_init_cond / pf_sampler_step_cond) ----
// The reference has no such call.  Two additions to its sample() (flow_model.py:229-374), both per residue:
//  * a PARTIAL START: the initial state is the training corruption's interpolant (flow_model.py:125-158) between the drawn noise and
//    a caller-given state at time ts[0], instead of the noise itself;
//  * ROW FLAGS and ALLOWED CLASSES: the three switches sample_bb / sample_ang / sample_seq per row (res_flags) and a 20-bit set of the
//    residue types that may be drawn on a row (aa_allowed).
// The bodies below are templates: COND = false is the unconstrained form, whose code does not read `c` at all.
template <bool COND>
__device__ __forceinline__ void row_flags(const pf_sampler_args& a, const pf_sampler_cond_args& c, size_t row, bool& f_bb, bool& f_an,
                                          bool& f_sq, uint32_t& allowed) {
    f_bb = a.sample_bb != 0; f_an = a.sample_ang != 0; f_sq = a.sample_seq != 0;
    allowed = ALL_CLASSES;
    if (COND) {
        if (c.res_flags) { const unsigned f = c.res_flags[row]; f_bb = f & 1u; f_an = (f >> 1) & 1u; f_sq = (f >> 2) & 1u; }
        if (c.aa_allowed) allowed = c.aa_allowed[row] & ALL_CLASSES;
    }
}

// ---- sampler init: flow_model.py:252-284, one workgroup per sample ----
template <bool COND>
__device__ __forceinline__ void sampler_init_entry(const pf_sampler_args& a, const pf_sampler_cond_args& c, const float* rot0, const float* tr0,
                                                   const float* ang0, const float* sx0) {
    __shared__ float red[4][4];
    const int b = blockIdx.x, L = a.L;
    const size_t rowb = (size_t)b * L;
    // Philox key from device memory when the caller says so (a captured graph is then reusable across sample() calls)
    const uint64_t seed = a.seed_dev ? a.seed_dev[0] : a.seed;
    const long long gs0 = a.sample_ids ? (long long)a.sample_ids[b] : (a.seed_dev ? (long long)a.seed_dev[1] : (long long)a.first_sample) + b;
    // centre of the generated residues (zero_center_part, flow_model.py:95-106)
    float sx = 0.f, sy = 0.f, sz = 0.f, cnt = 0.f;
    for (int l = threadIdx.x; l < L; l += 256) {
        const float gm = a.gen_mask[rowb + l];
        sx += tr0[(rowb + l) * 3 + 0] * gm; sy += tr0[(rowb + l) * 3 + 1] * gm; sz += tr0[(rowb + l) * 3 + 2] * gm;
        cnt += gm;
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz); cnt = wave_sum(cnt);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = sx; red[wave][1] = sy; red[wave][2] = sz; red[wave][3] = cnt; }
    __syncthreads();
    sx = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    sy = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    sz = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    cnt = red[0][3] + red[1][3] + red[2][3] + red[3][3];
    const float den = cnt + 1e-8f;
    const float cx = sx / den, cy = sy / den, cz = sz / den;
    for (int l = threadIdx.x; l < L; l += 256) {
        const size_t row = rowb + l;
        const bool gen = a.gen_mask[row] > 0.5f;
        const float rm = a.res_mask[row];
        bool f_bb, f_an, f_sq;
        uint32_t allowed;
        row_flags<COND>(a, c, row, f_bb, f_an, f_sq, allowed);
        const bool bb = gen && f_bb, an = gen && f_an, sq = gen && f_sq;
        // partial start: the interpolants of the training corruption (flow_model.py:131-155) at t0 = ts[0], base = the noise,
        // target = the caller's state; the noise itself stays in trans0 / simplex0 for the Euler steps (318, 328)
        const bool part = COND && c.partial != 0;
        const float t0 = part ? a.ts[0] : 0.f;
        if (part && bb) {
            float R0[9], R1s[9], Rt[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) { R0[k] = rot0[row * 9 + k]; R1s[k] = c.start_rot[row * 9 + k]; }
            so3_geodesic_dev(R0, R1s, t0, Rt);
#pragma unroll
            for (int k = 0; k < 9; ++k) a.rot_t[row * 9 + k] = Rt[k];
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) a.rot_t[row * 9 + k] = bb ? rot0[row * 9 + k] : a.rot1[row * 9 + k];
        }
        const float c3[3] = {cx, cy, cz};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = bb ? (tr0[row * 3 + k] - c3[k]) * rm : a.trans1[row * 3 + k];
            a.trans0[row * 3 + k] = v;
            a.trans_t[row * 3 + k] = (part && bb) ? (1.f - t0) * v + t0 * c.start_trans[row * 3 + k] : v;
        }
        const long long s1 = a.seq1[row];
        float lg[KCLS], lt[KCLS];
#pragma unroll
        for (int k = 0; k < KCLS; ++k) lg[k] = SIMPLEX_K * sx0[row * KCLS + k];
        const long long sst = (part && sq) ? (long long)c.start_seq[row] : 0;
#pragma unroll
        for (int k = 0; k < KCLS; ++k) lt[k] = (part && sq) ? (1.f - t0) * lg[k] + t0 * simplex_of(sst, k) : lg[k];
        long long s0 = s1;
        if (sq) s0 = categorical_dev<COND>(lt, a.expo ? a.expo + row * KCLS : nullptr, seed, gs0, 0, l, allowed);
        a.seq_t[row] = s0;
#pragma unroll
        for (int k = 0; k < KCLS; ++k) {
            a.simplex0[row * KCLS + k] = sq ? lg[k] : simplex_of(s1, k);
            a.simplex_t[row * KCLS + k] = sq ? lt[k] : simplex_of(s1, k);
        }
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            const float v0 = an ? ang0[row * 5 + d] : a.ang1[row * 5 + d];
            a.ang_t[row * 5 + d] = (part && an) ? tor_geodesic_dev(v0, c.start_ang[row * 5 + d], t0) : v0;      // (no torsion mask at init, as 262-267)
        }
    }
    if (threadIdx.x == 0) {
        a.t_out[b] = a.ts[0];
        if (b == 0) { a.step[0] = 0; a.step[1] = 0; }
    }
}
__global__ __launch_bounds__(256) void sampler_init_kernel(pf_sampler_args a, const float* rot0, const float* tr0, const float* ang0,
                                                           const float* sx0) {
    sampler_init_entry<false>(a, pf_sampler_cond_args{}, rot0, tr0, ang0, sx0);
}
__global__ __launch_bounds__(256) void sampler_init_cond_kernel(pf_sampler_args a, pf_sampler_cond_args c, const float* rot0, const float* tr0,
                                                                const float* ang0, const float* sx0) {
    sampler_init_entry<true>(a, c, rot0, tr0, ang0, sx0);
}

// ---- one sampler step: post-process (291-312 / 349-370), record, Euler (316-343) ----
// EIGHT lanes per residue: the three categorical draws are spread over them (categorical_oct); everything else is computed
// redundantly by the eight lanes and stored by lane 0.  (One thread per residue ran ~8 k dependent scalar instructions:
// 26 us per step on 4 workgroups at B*L = 1024.)
template <bool COND>
__device__ __forceinline__ void sampler_step_body(const pf_sampler_args& a, const pf_sampler_cond_args& c) {
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 3, sub = threadIdx.x & 7;
    const bool lead = sub == 0;
    const int n = a.B * a.L;
    if (row >= n) return;
    const int s = *a.step;
    if (s >= a.num_steps) return;
    const int b = row / a.L, l = row - b * a.L;
    const bool gen = a.gen_mask[row] > 0.5f;
    const size_t nrow = (size_t)n;
    const uint64_t seed = a.seed_dev ? a.seed_dev[0] : a.seed;
    const long long gs = a.sample_ids ? (long long)a.sample_ids[b] : (a.seed_dev ? (long long)a.seed_dev[1] : (long long)a.first_sample) + b;

    // -------- clean prediction --------
    float Rp[9], xp[3], angp[5], sxp[KCLS];
    bool f_bb, f_an, f_sq;                 // the row's switches (COND: res_flags, else a.sample_*) and its allowed classes
    uint32_t allowed;
    row_flags<COND>(a, c, (size_t)row, f_bb, f_an, f_sq, allowed);
    const bool bb = gen && f_bb;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rp[k] = bb ? a.pred_rot[(size_t)row * 9 + k] : a.rot1[(size_t)row * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) xp[k] = bb ? a.pred_trans[(size_t)row * 3 + k] : a.trans1[(size_t)row * 3 + k];
    const long long s1 = a.seq1[row];
    long long seqp = s1;
    long long seq_for_mask;
    if (COND) {
        // the row's flag is not uniform over the wave: ONE draw per generated row serves both uses below (same logits, same draw index)
        long long drawn = s1;
        if (gen) {
            float lg[KCLS];
#pragma unroll
            for (int k = 0; k < KCLS; ++k) lg[k] = a.pred_logits[(size_t)row * KCLS + k];
            const float* ex = a.expo ? a.expo + ((size_t)(1 + 2 * s) * nrow + row) * KCLS : nullptr;
            drawn = categorical_oct<COND>(lg, ex, seed, gs, 1 + 2 * s, l, sub, allowed);
        }
        seqp = f_sq ? drawn : s1;
        seq_for_mask = drawn;
    } else {
        if (gen && f_sq) {
            float lg[KCLS];
#pragma unroll
            for (int k = 0; k < KCLS; ++k) lg[k] = a.pred_logits[(size_t)row * KCLS + k];
            const float* ex = a.expo ? a.expo + ((size_t)(1 + 2 * s) * nrow + row) * KCLS : nullptr;
            seqp = categorical_oct(lg, ex, seed, gs, 1 + 2 * s, l, sub);
        }
        seq_for_mask = seqp;
        if (gen && !f_sq) {
            float lg[KCLS];
#pragma unroll
            for (int k = 0; k < KCLS; ++k) lg[k] = a.pred_logits[(size_t)row * KCLS + k];
            const float* ex = a.expo ? a.expo + ((size_t)(1 + 2 * s) * nrow + row) * KCLS : nullptr;
            seq_for_mask = categorical_oct(lg, ex, seed, gs, 1 + 2 * s, l, sub);
        }
    }
#pragma unroll
    for (int k = 0; k < KCLS; ++k) sxp[k] = simplex_of(seqp, k);
    // angles: where(gen, pred % 2pi, gt) ; then torsion mask of the drawn residue type (302-303).
    // NB the reference draws the sequence and applies its torsion mask even when sample_seq=False.
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        float v = gen ? py_mod_2pi(a.pred_ang_raw[(size_t)row * 5 + d]) : a.ang1[(size_t)row * 5 + d];
        if (!torsion_exists(seq_for_mask, d)) v = 0.f;
        if (!f_an) v = a.ang1[(size_t)row * 5 + d];
        angp[d] = v;
    }
    // record
    if (lead) {
        const size_t o = (size_t)s * nrow + row;
#pragma unroll
        for (int k = 0; k < 9; ++k) a.traj_rot[o * 9 + k] = Rp[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) a.traj_trans[o * 3 + k] = xp[k];
#pragma unroll
        for (int d = 0; d < 5; ++d) a.traj_ang[o * 5 + d] = angp[d];
        a.traj_seq[o] = seqp;
#pragma unroll
        for (int k = 0; k < KCLS; ++k) a.traj_simplex[o * KCLS + k] = sxp[k];
    }
    if (s == a.num_steps - 1) return;

    // -------- Euler step --------
    const float dt = a.ts[s + 1] - a.ts[s];
    // translations (318-320)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t o = (size_t)row * 3 + k;
        const float v = a.trans_t[o] + (xp[k] - a.trans0[o]) * dt;
        const float w = bb ? v : a.trans1[o];
        if (lead) a.trans_t[o] = w;
    }
    // rotations (322-323): geodesic with rate 10
    {
        float Rt[9], Rn[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rt[k] = a.rot_t[(size_t)row * 9 + k];
        if (bb) so3_geodesic_dev(Rt, Rp, dt * 10.f, Rn);
#pragma unroll
        for (int k = 0; k < 9; ++k) { const float w = bb ? Rn[k] : a.rot1[(size_t)row * 9 + k]; if (lead) a.rot_t[(size_t)row * 9 + k] = w; }
    }
    // simplex + state sequence (328-330)
    float lg[KCLS];
#pragma unroll
    for (int k = 0; k < KCLS; ++k) {
        const size_t o = (size_t)row * KCLS + k;
        lg[k] = a.simplex_t[o] + (sxp[k] - a.simplex0[o]) * dt;
    }
    long long seqn = s1;
    long long seqn_mask = s1;
    if (gen) {
        const float* ex = a.expo ? a.expo + ((size_t)(2 + 2 * s) * nrow + row) * KCLS : nullptr;
        seqn_mask = categorical_oct<COND>(lg, ex, seed, gs, 2 + 2 * s, l, sub, allowed);
        seqn = f_sq ? seqn_mask : s1;
    }
    // (the state is read by all eight lanes above and written only after the last read: wave-synchronous, lane 0 stores)
    if (lead) {
#pragma unroll
        for (int k = 0; k < KCLS; ++k) a.simplex_t[(size_t)row * KCLS + k] = lg[k];
        a.seq_t[row] = seqn;
    }
    // angles (325-326, 332-333)
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        const size_t o = (size_t)row * 5 + d;
        float v = gen ? tor_geodesic_dev(a.ang_t[o], angp[d], dt) : a.ang1[o];
        if (!torsion_exists(seqn_mask, d)) v = 0.f;
        if (!f_an) v = a.ang1[o];
        if (lead) a.ang_t[o] = v;
    }
}

// The step counter is bumped by the LAST workgroup to finish (ticket in step[1]): every workgroup has read step[0] long
// before it takes its ticket, so no workgroup can see the new value; the next kernel sees it through the kernel boundary.
// (A separate one-workgroup bump kernel cost a 4 us launch per step.)
template <bool COND>
__device__ __forceinline__ void sampler_step_entry(const pf_sampler_args& a, const pf_sampler_cond_args& c) {
    __shared__ int last;
    const int s0 = *a.step;
    sampler_step_body<COND>(a, c);
    __syncthreads();
    if (threadIdx.x == 0) last = (atomicAdd(a.step + 1, 1) == (int)gridDim.x - 1);
    __syncthreads();
    if (!last) return;
    const int s = s0 + 1;
    if (threadIdx.x == 0) { a.step[0] = s; a.step[1] = 0; }
    const int sc = s < a.num_steps ? s : a.num_steps - 1;
    for (int b = threadIdx.x; b < a.B; b += blockDim.x) a.t_out[b] = a.ts[sc];
}
// (two kernels, not one template: the unconstrained one keeps the kernel arguments it always had)
__global__ __launch_bounds__(256) void sampler_step_kernel(pf_sampler_args a) { sampler_step_entry<false>(a, pf_sampler_cond_args{}); }
__global__ __launch_bounds__(256) void sampler_step_cond_kernel(pf_sampler_args a, pf_sampler_cond_args c) { sampler_step_entry<true>(a, c); }

__global__ __launch_bounds__(256) void so3_geodesic_kernel(const float* base, const float* target, const float* t, float* out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float B[9], T[9], O[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { B[k] = base[(size_t)i * 9 + k]; T[k] = target[(size_t)i * 9 + k]; }
    so3_geodesic_dev(B, T, t[i], O);
#pragma unroll
    for (int k = 0; k < 9; ++k) out[(size_t)i * 9 + k] = O[k];
}
__global__ __launch_bounds__(256) void so3_log_kernel(const float* rot, float* w, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float M[9], v[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = rot[(size_t)i * 9 + k];
    so3_log_dev(M, v);
    w[(size_t)i * 3] = v[0]; w[(size_t)i * 3 + 1] = v[1]; w[(size_t)i * 3 + 2] = v[2];
}
__global__ __launch_bounds__(256) void so3_exp_kernel(const float* w, float* rot, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v[3] = {w[(size_t)i * 3], w[(size_t)i * 3 + 1], w[(size_t)i * 3 + 2]}, R[9];
    so3_exp_dev(v, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) rot[(size_t)i * 9 + k] = R[k];
}
__global__ __launch_bounds__(256) void torus_geodesic_kernel(const float* base, const float* target, const float* t, float* out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = tor_geodesic_dev(base[i], target[i], t[i]);
}

bool sampler_args_ok(const pf_sampler_args* a) {
    return a && a->rot1 && a->trans1 && a->ang1 && a->seq1 && a->gen_mask && a->res_mask && a->rot_t && a->trans_t &&
           a->ang_t && a->seq_t && a->simplex_t && a->trans0 && a->simplex0 && a->ts && a->step && a->t_out &&
           a->num_steps > 0 && a->B > 0 && a->L > 0;
}

bool cond_args_ok(const pf_sampler_cond_args* c) {   // NULL is a valid "no conditioning"; a partial start needs all four start tensors
    return !c || !c->partial || (c->start_rot && c->start_trans && c->start_ang && c->start_seq);
}
bool cond_planes_set(const pf_sampler_cond_args* c) { return c && (c->res_flags || c->aa_allowed); }

}  // namespace

extern "C" int pf_sampler_init(const pf_sampler_args* a, const float* rot0, const float* trans0_raw, const float* ang0,
                               const float* simplex0_raw, pf_stream_t stream) {
    return pf_sampler_init_cond(a, nullptr, rot0, trans0_raw, ang0, simplex0_raw, stream);
}

extern "C" int pf_sampler_step(const pf_sampler_args* a, pf_stream_t stream) { return pf_sampler_step_cond(a, nullptr, stream); }

// cond == NULL, or a struct that asks for nothing, runs the unconstrained instantiation: the bits of pf_sampler_init / pf_sampler_step
extern "C" int pf_sampler_init_cond(const pf_sampler_args* a, const pf_sampler_cond_args* c, const float* rot0, const float* trans0_raw,
                                    const float* ang0, const float* simplex0_raw, pf_stream_t stream) {
    if (!sampler_args_ok(a) || !cond_args_ok(c) || !rot0 || !trans0_raw || !ang0 || !simplex0_raw) return PF_E_BADARG;
    if (cond_planes_set(c) || (c && c->partial))
        hipLaunchKernelGGL(sampler_init_cond_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a, *c, rot0, trans0_raw, ang0, simplex0_raw);
    else
        hipLaunchKernelGGL(sampler_init_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a, rot0, trans0_raw, ang0, simplex0_raw);
    PF_CHECK_LAUNCH();
    return 0;
}

extern "C" int pf_sampler_step_cond(const pf_sampler_args* a, const pf_sampler_cond_args* c, pf_stream_t stream) {
    if (!sampler_args_ok(a) || !cond_args_ok(c) || !a->pred_rot || !a->pred_trans || !a->pred_ang_raw || !a->pred_logits || !a->traj_rot ||
        !a->traj_trans || !a->traj_ang || !a->traj_seq || !a->traj_simplex)
        return PF_E_BADARG;
    const int n = a->B * a->L;
    const dim3 grid((unsigned)((n + 31) / 32));
    if (cond_planes_set(c))                      // (a partial start is the init's business: the step is today's body with the row's flags)
        hipLaunchKernelGGL(sampler_step_cond_kernel, grid, dim3(256), 0, (hipStream_t)stream, *a, *c);
    else
        hipLaunchKernelGGL(sampler_step_kernel, grid, dim3(256), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}

#define PF_SIMPLE_LAUNCH(kern, n, ...)                                                                              \
    do {                                                                                                            \
        if ((n) <= 0) return PF_E_BADARG;                                                                           \
        hipLaunchKernelGGL(kern, dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__); \
        PF_CHECK_LAUNCH();                                                                                          \
        return 0;                                                                                                   \
    } while (0)

extern "C" int pf_so3_geodesic(const float* base, const float* target, const float* t, float* out, int n, pf_stream_t stream) {
    if (!base || !target || !t || !out) return PF_E_BADARG;
    PF_SIMPLE_LAUNCH(so3_geodesic_kernel, n, base, target, t, out, n);
}
extern "C" int pf_so3_log(const float* rot, float* rotvec, int n, pf_stream_t stream) {
    if (!rot || !rotvec) return PF_E_BADARG;
    PF_SIMPLE_LAUNCH(so3_log_kernel, n, rot, rotvec, n);
}
extern "C" int pf_so3_exp(const float* rotvec, float* rot, int n, pf_stream_t stream) {
    if (!rotvec || !rot) return PF_E_BADARG;
    PF_SIMPLE_LAUNCH(so3_exp_kernel, n, rotvec, rot, n);
}
extern "C" int pf_torus_geodesic(const float* base, const float* target, const float* t, float* out, int n, pf_stream_t stream) {
    if (!base || !target || !t || !out) return PF_E_BADARG;
    PF_SIMPLE_LAUNCH(torus_geodesic_kernel, n, base, target, t, out, n);
}
