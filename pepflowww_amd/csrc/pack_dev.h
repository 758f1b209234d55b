// Device helpers shared by packing.hip, mutscan.hip and seqdesign.hip: the pair function, the backbone frame with the chi1 offset, the rotamer frame
// chain and a residue's environment atoms.  Pure functions of their arguments; `Args` is pf_pack_args, pf_mutation_scan_args or pf_sequence_design_args, which
// name the tables, the rotamer table and the weights alike.  The conventions and the summation order are stated in packing.hip; the
// operation order here is the one its oracle (tests/pack_oracle.py) restates, so nothing in this file may be reassociated.
#pragma once
#include "common.h"
#include "../../include/pepflow_hip.h"
#include "eval_dev.h"

namespace pack_dev {

constexpr int SL = PF_PACK_SLOTS, RA = PF_PACK_ROT_ATOMS, S0 = 5;      // slots per residue, rotamer atoms per residue, their first slot
constexpr int MAXR = PF_PACK_MAX_ROT, MAXN = PF_PACK_MAX_N;
constexpr int TR = 16, TA = TR * SL, NT = 256;                          // environment tile: residues, atoms; threads
constexpr int MAX_TILES = MAXN / TR;
constexpr float FAR = 1e18f;
constexpr float CULL_SLACK = 1.0001f, CULL_ABS = 1e-3f;
constexpr unsigned char HYDROPHOBIC = 1, DONOR = 2, ACCEPTOR = 4, IS_SG = 8;

__device__ __forceinline__ float dist3(const float4& p, const float4& q) {
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// the pair function of interface_energy.hip's energy_kernel: the five terms of the pair (P, v) when it is inside the cutoff
__device__ __forceinline__ bool pair_terms(const float4& P, unsigned char fp, const float4& v, unsigned char fv, float cut2, float o[5]) {
    const float dx = P.x - v.x, dy = P.y - v.y, dz = P.z - v.z;
    const float r2 = (dx * dx + dy * dy) + dz * dz;
    if (!(r2 < cut2)) return false;
    const float d = sqrtf(r2) - (P.w + v.w);
    const float g1 = d * 2.f, g2 = (d - 3.f) * 0.5f;
    o[0] = expf(-(g1 * g1));
    o[1] = expf(-(g2 * g2));
    o[2] = d < 0.f ? d * d : 0.f;
    const bool hp = (fp & HYDROPHOBIC) && (fv & HYDROPHOBIC);
    const bool hb = ((fp & DONOR) && (fv & ACCEPTOR)) || ((fp & ACCEPTOR) && (fv & DONOR));
    o[3] = !hp ? 0.f : d <= 0.5f ? 1.f : d >= 1.5f ? 0.f : 1.5f - d;
    o[4] = !hb ? 0.f : d <= -0.7f ? 1.f : d >= 0.f ? 0.f : d * (-1.f / 0.7f);
    return true;
}

// adds the pair (P, v) to the five sums when it is inside the cutoff
__device__ __forceinline__ void pair_add(const float4& P, unsigned char fp, const float4& v, unsigned char fv, float cut2, float t[5]) {
    float o[5];
    if (pair_terms(P, fp, v, fv, cut2, o)) {
#pragma unroll
        for (int k = 0; k < 5; ++k) t[k] += o[k];
    }
}

template <class Args>
__device__ __forceinline__ float weighted(const Args& a, const float t[5]) {
    return (((a.w_gauss1 * t[0] + a.w_gauss2 * t[1]) + a.w_repulsion * t[2]) + a.w_hydrophobic * t[3]) + a.w_hbond * t[4];
}

template <class Args>
__device__ __forceinline__ int rot_count(const Args& a, int t) {
    const int c = a.rot_count[t];
    return c < 1 ? 1 : c > a.max_rot ? a.max_rot : c;
}

// (value, index) total order of the argmins; NaN was mapped to +inf by the caller
__device__ __forceinline__ bool better(float v, int i, float v2, int i2) { return v < v2 || (v == v2 && i < i2); }

__device__ __forceinline__ float no_nan(float v) { return v == v ? v : INFINITY; }

__device__ __forceinline__ void apply(const float R[9], const float t[3], const float q[3], float o[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = R[i * 3] * q[0] + R[i * 3 + 1] * q[1] + R[i * 3 + 2] * q[2] + t[i];
}

// (R, t) = (R1, t1) o (R2, t2), as full_atom.hip composes
__device__ __forceinline__ void compose(const float* R1, const float* t1, const float* R2, const float* t2, float* R, float* t) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = R1[i * 3] * R2[j] + R1[i * 3 + 1] * R2[3 + j] + R1[i * 3 + 2] * R2[6 + j];
        t[i] = R1[i * 3] * t2[0] + R1[i * 3 + 1] * t2[1] + R1[i * 3 + 2] * t2[2] + t1[i];
    }
}

// the frame of a residue's own backbone, the CB of type t in it, and the chi1 offset of type t
struct Backbone {
    float R[9], t[3], cb[3], chi1_eps;
};

// p: the residue's atoms (N, CA, C first); on: the residue is built on (else everything stays zero)
template <class Args>
__device__ __forceinline__ void backbone_frame(const Args& a, int t, const float* p, bool on, Backbone& F) {
#pragma unroll
    for (int k = 0; k < 9; ++k) F.R[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) F.t[k] = F.cb[k] = 0.f;
    F.chi1_eps = 0.f;
    if (!on) return;
    float u[3], v[3], e1[3], e2[3], e3[3];                  // construct_3d_basis(CA, C, N)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        F.t[k] = p[3 + k];
        u[k] = p[6 + k] - p[3 + k];
        v[k] = p[k] - p[3 + k];
    }
    const float lu = sqrtf((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + 1e-6f;
#pragma unroll
    for (int k = 0; k < 3; ++k) e1[k] = u[k] / lu;
    const float pr = (e1[0] * v[0] + e1[1] * v[1]) + e1[2] * v[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = v[k] - pr * e1[k];
    const float lv = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 1e-6f;
#pragma unroll
    for (int k = 0; k < 3; ++k) e2[k] = v[k] / lv;
    e3[0] = e1[1] * e2[2] - e1[2] * e2[1];
    e3[1] = e1[2] * e2[0] - e1[0] * e2[2];
    e3[2] = e1[0] * e2[1] - e1[1] * e2[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        F.R[k * 3] = e1[k];
        F.R[k * 3 + 1] = e2[k];
        F.R[k * 3 + 2] = e3[k];
    }
    apply(F.R, F.t, a.tab_pos + ((size_t)t * 14 + 4) * 3, F.cb);
    // chi1 is the dihedral N-CA-CB-CG from the REAL N; the chain turns from where the ideal N is.  In the backbone frame both lie
    // in the e1-e2 plane; eps = the signed angle about CA-CB from the real N's projection to the ideal N's.
    if (a.tab_mask[t * SL + 4]) {
        const float* q = a.tab_pos + ((size_t)t * 14 + 4) * 3;
        const float* ni = a.tab_pos + (size_t)t * 14 * 3;
        const float nr[3] = {pr, (e2[0] * v[0] + e2[1] * v[1]) + e2[2] * v[2], 0.f};
        const float lq = sqrtf((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
        if (lq > 0.f) {
            const float ax[3] = {q[0] / lq, q[1] / lq, q[2] / lq};
            const float dr = (nr[0] * ax[0] + nr[1] * ax[1]) + nr[2] * ax[2], di = (ni[0] * ax[0] + ni[1] * ax[1]) + ni[2] * ax[2];
            const float pa[3] = {nr[0] - dr * ax[0], nr[1] - dr * ax[1], nr[2] - dr * ax[2]};
            const float pb[3] = {ni[0] - di * ax[0], ni[1] - di * ax[1], ni[2] - di * ax[2]};
            const float cx[3] = {pa[1] * pb[2] - pa[2] * pb[1], pa[2] * pb[0] - pa[0] * pb[2], pa[0] * pb[1] - pa[1] * pb[0]};
            const float y = (ax[0] * cx[0] + ax[1] * cx[1]) + ax[2] * cx[2], x = (pa[0] * pb[0] + pa[1] * pb[1]) + pa[2] * pb[2];
            const float e = atan2f(y, x);
            if (e == e) F.chi1_eps = e;
        }
    }
}

// One rotamer of type t on the backbone F: the frame chain chi1 .. chi4 (chi: the table row), emit(j, atom) for every rotamer atom
// j (slot 5 + j) the type has, frame by frame and slots ascending in a frame.  -> the largest distance of an emitted atom from CA.
template <class Args, class Emit>
__device__ __forceinline__ float build_rotamer(const Args& a, int t, const float* chi, const Backbone& F, Emit emit) {
    float ext = 0.f;
    float Rc[9], tc[3];                                     // the current frame: the backbone's, then chi1 .. chi4
#pragma unroll
    for (int k = 0; k < 9; ++k) Rc[k] = F.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tc[k] = F.t[k];
    const float zero3[3] = {0.f, 0.f, 0.f};
    const float4 ca = make_float4(F.t[0], F.t[1], F.t[2], 0.f);
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const float ang = f == 0 ? chi[0] - F.chi1_eps : chi[f];
        const float sn = sinf(ang), cs = cosf(ang);
        const float Rx[9] = {1.f, 0.f, 0.f, 0.f, cs, -sn, 0.f, sn, cs};
        const float* Rg = a.tab_rot + ((size_t)t * 8 + 4 + f) * 9;
        const float* tg = a.tab_trans + ((size_t)t * 8 + 4 + f) * 3;
        float Rm[9], tm[3], Rn[9], tn[3];
        compose(Rg, tg, Rx, zero3, Rm, tm);
        compose(Rc, tc, Rm, tm, Rn, tn);
#pragma unroll
        for (int k = 0; k < 9; ++k) Rc[k] = Rn[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tc[k] = tn[k];
        for (int j = 0; j < RA; ++j) {                      // the atoms of this frame's rigid group
            const int s = S0 + j;
            if (a.tab_group[t * 14 + s] != 4 + f || !a.tab_mask[t * SL + s]) continue;
            float x[3];
            apply(Rc, tc, a.tab_pos + ((size_t)t * 14 + s) * 3, x);
            const float4 o = make_float4(x[0], x[1], x[2], a.radius[t * SL + s]);
            ext = fmaxf(ext, dist3(o, ca));
            emit(j, o);
        }
    }
    return ext;
}

// The 15 environment atoms of a residue of type row t as float4 (x, y, z, radius; an absent one parked at x = -FAR, radius 0) and
// their type bytes (bit 3: CYS SG).  built: N, CA, C, O and slot 14 as given, CB = cb (the type's, rebuilt), no other side-chain
// atom; else every existing atom as given.  m, p: the residue's atom_mask and pos rows of A slots.
template <class Args>
__device__ __forceinline__ void env_atoms(const Args& a, int t, const unsigned char* m, const float* p, int A, bool built, const float cb[3],
                                          float4 e[SL], unsigned char flg[SL]) {
    for (int s = 0; s < SL; ++s) {
        const float rad = a.radius[t * SL + s];
        const bool input = s < A && m[s] != 0 && rad > 0.f;
        e[s] = make_float4(-FAR, 0.f, 0.f, 0.f);
        if (built && s == 4) {
            if (a.tab_mask[t * SL + 4] && rad > 0.f) e[s] = make_float4(cb[0], cb[1], cb[2], rad);
        } else if (input && (!built || s < 4 || s == 14)) {
            e[s] = make_float4(p[3 * s], p[3 * s + 1], p[3 * s + 2], rad);
        }
        flg[s] = (unsigned char)(a.types[t * SL + s] | (t == a.cys && s == S0 ? IS_SG : 0));
    }
}

// centre (CA, else the first existing atom) and extent of a residue's environment atoms; w = -1: it has none
__device__ __forceinline__ float4 env_bound(const float4 e[SL]) {
    int c = e[1].w > 0.f ? 1 : -1;
    for (int s = 0; s < SL && c < 0; ++s)
        if (e[s].w > 0.f) c = s;
    float4 bd = make_float4(0.f, 0.f, 0.f, -1.f);
    if (c >= 0) {
        bd = make_float4(e[c].x, e[c].y, e[c].z, 0.f);
        for (int s = 0; s < SL; ++s)
            if (e[s].w > 0.f) bd.w = fmaxf(bd.w, dist3(e[s], bd));
    }
    return bd;
}

// is the tile of residues [c0, c1) of a sample to be visited from the sphere C (centre, extent)?  ebound: the sample's env_bound()s
__device__ __forceinline__ bool tile_near(const float4* ebound, int c0, int c1, const float4& C, float cutoff) {
    bool keep = false;
    for (int c = c0; c < c1; ++c) {
        const float4 e = ebound[c];
        keep = keep || (e.w >= 0.f && dist3(e, C) <= ((C.w + e.w) + cutoff) * CULL_SLACK + CULL_ABS);
    }
    return keep;
}

}  // namespace pack_dev
