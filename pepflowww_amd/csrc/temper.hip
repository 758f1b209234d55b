// Tempered and stochastic sampling: the sequence temperature and the noise on the backbone state of one sampler step
// (pf_sampler_temper; formulas and conventions: include/pepflow_hip.h).  The reference has no such call.
//
// One thread per row, one launch per step between the network (and pf_guidance_fwd) and the step kernel.  Part a) writes the logits
// divided by the row's temperature into a buffer the step kernel is pointed at; part b) perturbs rot_t / trans_t of the movable rows
// before the step kernel takes its Euler step from them.  The normals are the caller's (gauss) or Philox4x32-10 draws with the
// sampler's key; the counter's word 1 carries the high bit, which no categorical draw uses, so the streams stay apart.  A thread reads
// and writes its own row only: no barrier, no shared memory, and a row gives the same bits in any batch and at any padded length.
#include "common.h"
#include "flow_dev.h"
#include "../../include/pepflow_hip.h"

namespace {

constexpr float U24 = 5.9604644775390625e-08f;                 // 2^-24: u = ((c >> 8) + 0.5) * 2^-24 lies in (0, 1), as categorical_dev

// Box-Muller on one pair of uniforms
__device__ __forceinline__ void box_muller(uint32_t ca, uint32_t cb, float& z0, float& z1) {
    const float ua = ((float)(ca >> 8) + 0.5f) * U24, ub = ((float)(cb >> 8) + 0.5f) * U24;
    const float r = sqrtf(-2.f * logf(ua));
    const float ang = TWO_PI_F * ub;
    z0 = r * cosf(ang);
    z1 = r * sinf(ang);
}

__global__ __launch_bounds__(256) void sampler_temper_kernel(const pf_sampler_temper_args a) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    const int n = a.B * a.L;
    if (row >= n) return;
    const int s = a.step[0];
    if (s >= a.num_steps) return;                              // (uniform over the grid: the step kernel returns the same way)
    const size_t r = (size_t)row;

    // ---- a) tempered logits: every row, every step ----
    if (a.tau) {
        const float tau = a.tau[r];
#pragma unroll
        for (int k = 0; k < KCLS; ++k) a.tempered_logits[r * KCLS + k] = a.pred_logits[r * KCLS + k] / tau;
    }

    // ---- b) noise on the backbone state of the movable rows, not on the record-only last step ----
    if (!a.params || s >= a.num_steps - 1) return;
    const bool f_bb = a.res_flags ? (a.res_flags[r] & 1u) != 0 : a.sample_bb != 0;
    if (!(a.gen_mask[r] > 0.5f) || !f_bb) return;
    const float sigma_trans = a.params[0], sigma_rot = a.params[1], t_off = a.params[3];
    const int power = (int)a.params[2];
    const float t = a.ts[s], dt = a.ts[s + 1] - a.ts[s];
    const float u = 1.f - t;
    const float w = power == 0 ? 1.f : power == 1 ? u : u * u;
    const float sc = t >= t_off ? 0.f : sqrtf(dt) * w;
    const float st = sigma_trans * sc, sr = sigma_rot * sc;
    if (st == 0.f && sr == 0.f) return;

    float z[6];
    if (a.gauss) {
        const float* g = a.gauss + ((size_t)s * (size_t)n + r) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) z[k] = g[k];
    } else {
        const int b = row / a.L, l = row - b * a.L;
        const uint64_t seed = a.seed_dev ? a.seed_dev[0] : a.seed;
        const long long gs = a.sample_ids ? (long long)a.sample_ids[b] : (a.seed_dev ? (long long)a.seed_dev[1] : (long long)a.first_sample) + b;
        uint32_t c0[4] = {(uint32_t)(l * 2), 0x80000000u | (uint32_t)s, (uint32_t)gs, (uint32_t)((uint64_t)gs >> 32)};
        uint32_t c1[4] = {(uint32_t)(l * 2 + 1), 0x80000000u | (uint32_t)s, (uint32_t)gs, (uint32_t)((uint64_t)gs >> 32)};
        philox4x32_10(c0, (uint32_t)seed, (uint32_t)(seed >> 32));
        philox4x32_10(c1, (uint32_t)seed, (uint32_t)(seed >> 32));
        box_muller(c0[0], c0[1], z[0], z[1]);
        box_muller(c0[2], c0[3], z[2], z[3]);
        box_muller(c1[0], c1[1], z[4], z[5]);
    }
    if (st != 0.f) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.trans_t[r * 3 + k] += st * z[k];
    }
    if (sr != 0.f) {
        float R[9], E[9];
        const float v[3] = {sr * z[3], sr * z[4], sr * z[5]};
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = a.rot_t[r * 9 + k];
        so3_exp_dev(v, E);
        // rot_t * Exp(v): the explicit product of so3_geodesic_dev
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                a.rot_t[r * 9 + i * 3 + k] = R[i * 3 + 0] * E[0 * 3 + k] + R[i * 3 + 1] * E[1 * 3 + k] + R[i * 3 + 2] * E[2 * 3 + k];
    }
}

}  // namespace

extern "C" int pf_sampler_temper(const pf_sampler_temper_args* a, pf_stream_t stream) {
    if (!a || !a->step || !a->ts || a->num_steps <= 0 || a->B <= 0 || a->L <= 0) return PF_E_BADARG;
    if (!a->tau && !a->params) return PF_E_BADARG;                                      // nothing to do
    if (a->tau && (!a->pred_logits || !a->tempered_logits)) return PF_E_BADARG;
    if (a->params && (!a->rot_t || !a->trans_t || !a->gen_mask)) return PF_E_BADARG;
    if (a->gauss && !a->params) return PF_E_BADARG;
    const int n = a->B * a->L;
    hipLaunchKernelGGL(sampler_temper_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
