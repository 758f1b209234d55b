// pf_torsions_fwd, pf_sidechain_compare_fwd -- torsion angles of a batch of heavy-atom structures and the side-chain packing
// comparison of pairs of them (the chi1-chi4 errors and the share of residues with every chi within a tolerance that the
// reference's paper tabulates; the reference's own eval/geometry.py stops at `get_dihedral(): #TODO`).
//
// Conventions (tests/torsion_oracle.py restates them in numpy float64):
//   Atoms     slots 0..13 of pos [B,N,n_atoms,3] in the package's heavy-atom order (N, CA, C, O, CB, ...); slots >= 14 are not read.
//   Angles    slot 0 omega  CA(n-1), C(n-1), N, CA       slot 1 phi  C(n-1), N, CA, C       slot 2 psi  N, CA, C, N(n+1)
//             slot 3 psi_o  N, CA, C, O  -- slot 0 of preprocess.get_torsion_angle.  The model's first angle is psi_o - pi (mod 2 pi):
//                    full-atom reconstruction mirrors that torsion, measuring it from the atoms does not, and neither is changed here.
//             slots 4..7 chi1..chi4, the four atom slots of chi_atoms [21,4,4] (data/chi_atoms.npz; -1: the type has no such angle).
//   Dihedral  of p0, p1, p2, p3: b0 = p0 - p1, b1 = p2 - p1, b2 = p3 - p2, u = b1 / |b1|, v = b0 - (b0.u) u, w = b2 - (b2.u) u (the
//             parts of the outer bonds perpendicular to the central one), angle = atan2(u.(v x w), v.w) brought to [0, 2 pi): the sign
//             of `_dihedral` in preprocess.py ((b0 x b2).b1), 0 for cis, pi for trans.  fp32, from coordinate differences only, so a
//             translation that keeps the differences exact changes no bit.
//   Defined   all four atoms in atom_mask; for omega / phi the previous and for psi the next residue is bonded: residue_index grows by
//             exactly 1 (without residue_index: consecutive positions are bonded); chi: the type is 0..19 and has the angle (a type
//             outside 0..20 reads row 20, which has none); |b1|, |v| and |w| are all > 0.  Undefined: angle 0, defined 0, never NaN.
//   Compare   pair p = (i, j): x[i] against y[j].  Residue n, angle slot k is compared when both are defined and, for k >= 3, the two
//             types are equal and in 0..19.  error = |a_x - a_y| wrapped to [0, pi]; where periodic[type][k - 4] is set (a chi whose
//             two end atoms are equivalent: ASP chi2, GLU chi3, PHE chi2, TYR chi2) wrapped to [0, pi/2].  fp32 per angle, summed in fp64.
//             err_sum / err_count / within (error <= correct_tol) per slot; res_with_chi counts residues with a compared chi,
//             res_correct those whose compared chi are all within correct_tol.
//   Frame     side-chain deviation: slots 4..13 of each structure in its own backbone frame, origin CA, e1 = unit(C - CA), e2 =
//             unit(N - CA made orthogonal to e1), e3 = e1 x e2, no epsilon; a residue without N, CA or C in either mask, or with a
//             zero-length e1 / e2, is left out.  For equal types in 0..19 the squared differences are summed over the slots in both
//             masks.  swap[type] = (a1, b1, a2, b2) lists up to two slot pairs (0, 0: unused) that are equivalent (ASP OD1/OD2, GLU
//             OE1/OE2, PHE and TYR CD1/CD2 with CE1/CE2); when every listed slot is in both masks the sum is also taken with x's slots
//             exchanged and the smaller kept (a tie keeps the unexchanged one).  fp32 per residue, fp64 over the pair.
//
// pf_torsions_fwd: one launch, grid (tiles of 64 residues, B), 256 threads.  The residue records (168 bytes at n_atoms = 14) are never
// read a lane per record: the tile and one halo residue on each side are staged in LDS by loads whose consecutive lanes read consecutive
// dwords (the 42 floats of a record's slots 0..13, records back to back), in rows of 43 dwords so that 64 lanes reading the same slot
// of 64 residues fall on distinct banks.  Wave w then computes angle slots w and w + 4 of the tile's 64 residues (uniform control flow
// for the backbone angles), the results go through LDS and leave as 8- and 4-byte stores of consecutive lanes.  No scratch memory.
// pf_sidechain_compare_fwd: one launch, one workgroup of 128 threads per pair, looping over N in tiles of 128 residues staged the
// same way, a thread per residue.  Every sum has a fixed order (a thread's residues ascending, lanes by a shuffle tree, wave 0 + wave
// 1); the only atomics are integer counters in LDS.  One writer per output: bit-identical from run to run and independent of the list.
#include "common.h"
#include "../../include/pepflow_hip.h"
#include "eval_dev.h"

namespace {

constexpr int SL = 14, REC = SL * 3;        // slots and floats read of a residue record
constexpr int RS = 43;                      // LDS row stride in dwords (odd: conflict-free across residues)
constexpr int MS = 16;                      // LDS mask row stride in bytes
constexpr int NA = 8;                       // angle slots
constexpr float PI_F = 3.14159274f, TWO_PI_F = 6.28318548f, HALF_PI_F = 1.57079637f;

// rows [first, first + rows) of sample `b` -> LDS; rows outside [0, N) get an all-zero mask and their coordinates are left alone
__device__ __forceinline__ void stage_rows(const float* pos, const unsigned char* mask, size_t b, int N, int n_atoms, int first, int rows,
                                           float* sp, unsigned char* sm, int tid, int nt) {
    for (int i = tid; i < rows * REC; i += nt) {
        const int h = i / REC, j = i - h * REC, n = first + h;
        if (n >= 0 && n < N) sp[h * RS + j] = pos[(b * N + n) * (size_t)n_atoms * 3 + j];
    }
    for (int i = tid; i < rows * SL; i += nt) {
        const int h = i / SL, s = i - h * SL, n = first + h;
        sm[h * MS + s] = (n >= 0 && n < N) ? (mask[(b * N + n) * (size_t)n_atoms + s] != 0) : 0;
    }
}


// the dihedral of four staged points; false where it is not defined (the value is then not used)
__device__ __forceinline__ bool dihedral(const float* p0, const float* p1, const float* p2, const float* p3, float& angle) {
    const float b0x = p0[0] - p1[0], b0y = p0[1] - p1[1], b0z = p0[2] - p1[2];
    const float b1x = p2[0] - p1[0], b1y = p2[1] - p1[1], b1z = p2[2] - p1[2];
    const float b2x = p3[0] - p2[0], b2y = p3[1] - p2[1], b2z = p3[2] - p2[2];
    const float l1 = sqrtf((b1x * b1x + b1y * b1y) + b1z * b1z);
    const float ux = b1x / l1, uy = b1y / l1, uz = b1z / l1;
    const float t0 = (b0x * ux + b0y * uy) + b0z * uz, t2 = (b2x * ux + b2y * uy) + b2z * uz;
    const float vx = b0x - t0 * ux, vy = b0y - t0 * uy, vz = b0z - t0 * uz;
    const float wx = b2x - t2 * ux, wy = b2y - t2 * uy, wz = b2z - t2 * uz;
    const float vv = (vx * vx + vy * vy) + vz * vz, ww = (wx * wx + wy * wy) + wz * wz;
    const float cx = vy * wz - vz * wy, cy = vz * wx - vx * wz, cz = vx * wy - vy * wx;
    const float y = (ux * cx + uy * cy) + uz * cz, x = (vx * wx + vy * wy) + vz * wz;
    float a = atan2f(y, x);
    if (a < 0.f) a += TWO_PI_F;
    if (a >= TWO_PI_F) a = 0.f;
    angle = a + 0.f;        // (atan2f gives -0 for y = -0, x > 0: store +0)
    return l1 > 0.f && vv > 0.f && ww > 0.f && a == a;
}

constexpr int TR = 64, HR = TR + 2, NT = 256;

__global__ __launch_bounds__(NT) void torsions_kernel(pf_torsions_args a) {
    __shared__ float sp[HR * RS];
    __shared__ unsigned char sm[HR * MS];
    __shared__ int sidx[HR], saa[HR];
    __shared__ int schi[21 * 16];
    __shared__ __attribute__((aligned(16))) float sang[TR * NA];
    __shared__ __attribute__((aligned(16))) unsigned char sdef[TR * NA];
    const int N = a.N, tid = threadIdx.x;
    const size_t b = blockIdx.y;
    const int r0 = blockIdx.x * TR;

    stage_rows(a.pos, a.atom_mask, b, N, a.n_atoms, r0 - 1, HR, sp, sm, tid, NT);
    if (tid < HR) {
        const int n = r0 - 1 + tid;
        const bool in = n >= 0 && n < N;
        sidx[tid] = in ? (a.residue_index ? a.residue_index[b * N + n] : n) : 0;
        saa[tid] = in ? type_row(a.aa[b * N + n]) : 20;
    }
    for (int i = tid; i < 21 * 16; i += NT) schi[i] = a.chi_atoms[i];
    __syncthreads();

    const int l = tid & 63, w = tid >> 6, h = l + 1;
    const bool in = r0 + l < N;
    const bool bond_prev = (long long)sidx[h] - (long long)sidx[h - 1] == 1;
    const bool bond_next = (long long)sidx[h + 1] - (long long)sidx[h] == 1;
    const int type = saa[h];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int k = w + 4 * pass;                         // uniform over the wave
        int hr[4], sl[4];
        bool ok = in;
        if (k == 0) {
            hr[0] = h - 1; sl[0] = 1; hr[1] = h - 1; sl[1] = 2; hr[2] = h; sl[2] = 0; hr[3] = h; sl[3] = 1;
            ok = ok && bond_prev;
        } else if (k == 1) {
            hr[0] = h - 1; sl[0] = 2; hr[1] = h; sl[1] = 0; hr[2] = h; sl[2] = 1; hr[3] = h; sl[3] = 2;
            ok = ok && bond_prev;
        } else if (k == 2) {
            hr[0] = h; sl[0] = 0; hr[1] = h; sl[1] = 1; hr[2] = h; sl[2] = 2; hr[3] = h + 1; sl[3] = 0;
            ok = ok && bond_next;
        } else if (k == 3) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { hr[j] = h; sl[j] = j; }
        } else {
            ok = ok && type < 20;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int s = schi[type * 16 + (k - 4) * 4 + j];
                const bool has = s >= 0 && s < SL;
                ok = ok && has;
                hr[j] = h;
                sl[j] = has ? s : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ok = ok && sm[hr[j] * MS + sl[j]] != 0;
        float ang = 0.f;
        if (ok) ok = dihedral(sp + hr[0] * RS + sl[0] * 3, sp + hr[1] * RS + sl[1] * 3, sp + hr[2] * RS + sl[2] * 3,
                              sp + hr[3] * RS + sl[3] * 3, ang);
        sang[l * NA + k] = ok ? ang : 0.f;
        sdef[l * NA + k] = ok;
    }
    __syncthreads();

    // thread t: floats 2t, 2t + 1 of the tile's [64,8] angles (residue t / 4); thread t < 128: bytes 4t .. 4t + 3 (residue t / 2)
    const size_t base = (b * N + r0) * NA;
    if (r0 + tid / 4 < N) reinterpret_cast<float2*>(a.angles + base)[tid] = reinterpret_cast<const float2*>(sang)[tid];
    if (tid < TR * NA / 4 && r0 + tid / 2 < N)
        reinterpret_cast<uchar4*>(a.defined + base)[tid] = reinterpret_cast<const uchar4*>(sdef)[tid];
}

// ---- comparison ----------------------------------------------------------------------------------------------------------------------

constexpr int CT = 128;                     // residues per tile = threads per pair

struct Frame {
    float o[3], e1[3], e2[3], e3[3];
    bool ok;
};

__device__ __forceinline__ Frame backbone_frame(const float* rec, const unsigned char* m) {
    Frame f;
    const float* n = rec;
    const float* ca = rec + 3;
    const float* c = rec + 6;
    float u[3], v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f.o[k] = ca[k];
        u[k] = c[k] - ca[k];
        v[k] = n[k] - ca[k];
    }
    const float lu = sqrtf((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) f.e1[k] = u[k] / lu;
    const float t = (v[0] * f.e1[0] + v[1] * f.e1[1]) + v[2] * f.e1[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = v[k] - t * f.e1[k];
    const float lv = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) f.e2[k] = v[k] / lv;
    f.e3[0] = f.e1[1] * f.e2[2] - f.e1[2] * f.e2[1];
    f.e3[1] = f.e1[2] * f.e2[0] - f.e1[0] * f.e2[2];
    f.e3[2] = f.e1[0] * f.e2[1] - f.e1[1] * f.e2[0];
    f.ok = m[0] && m[1] && m[2] && lu > 0.f && lv > 0.f;
    return f;
}

__device__ __forceinline__ void to_local(const Frame& f, const float* p, float out[3]) {
    const float d0 = p[0] - f.o[0], d1 = p[1] - f.o[1], d2 = p[2] - f.o[2];
    out[0] = (d0 * f.e1[0] + d1 * f.e1[1]) + d2 * f.e1[2];
    out[1] = (d0 * f.e2[0] + d1 * f.e2[1]) + d2 * f.e2[2];
    out[2] = (d0 * f.e3[0] + d1 * f.e3[1]) + d2 * f.e3[2];
}

// the sum over a wave in a fixed order (a shuffle tree), valid in lane 0
__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(CT) void sidechain_compare_kernel(pf_sidechain_compare_args a) {
    __shared__ float spx[CT * RS], spy[CT * RS];
    __shared__ unsigned char smx[CT * MS], smy[CT * MS];
    __shared__ int icnt[2 * NA + 3];                        // err_count[8], within[8], res_with_chi, res_correct, sc_atoms
    __shared__ double dsum[2][NA + 1];                      // per wave: err_sum[8], sc_sq_sum
    const int N = a.N, tid = threadIdx.x;
    const size_t p = blockIdx.x;
    const int pi = a.pairs[2 * p], pj = a.pairs[2 * p + 1];
    const bool valid = pi >= 0 && pi < a.Bx && pj >= 0 && pj < a.By;       // uniform over the workgroup
    const size_t i = valid ? pi : 0, j = valid ? pj : 0;
    const float tol = a.correct_tol;

    if (tid < 2 * NA + 3) icnt[tid] = 0;
    double esum[NA], sq_sum = 0.0;
    int ecnt[NA], ewin[NA], n_chi = 0, n_correct = 0, n_atoms_cmp = 0;
#pragma unroll
    for (int k = 0; k < NA; ++k) { esum[k] = 0.0; ecnt[k] = 0; ewin[k] = 0; }

    for (int r0 = 0; r0 < N; r0 += CT) {
        __syncthreads();                                    // the previous tile has been read
        if (valid) {
            stage_rows(a.pos_x, a.mask_x, i, N, a.n_atoms_x, r0, CT, spx, smx, tid, CT);
            stage_rows(a.pos_y, a.mask_y, j, N, a.n_atoms_y, r0, CT, spy, smy, tid, CT);
        }
        __syncthreads();
        const int n = r0 + tid;
        if (n >= N) continue;                               // (no barrier below this line inside the loop body)
        float err[NA];
        float sc = 0.f;
        int sc_n = 0;
        bool swapped = false;
#pragma unroll
        for (int k = 0; k < NA; ++k) err[k] = __builtin_nanf("");
        if (valid) {
            const size_t rx = i * N + n, ry = j * N + n;
            const int tx = type_row(a.aa_x[rx]), ty = type_row(a.aa_y[ry]);
            const bool same = tx == ty && tx < 20;
            const float4 ax0 = reinterpret_cast<const float4*>(a.angles_x + rx * NA)[0], ax1 = reinterpret_cast<const float4*>(a.angles_x + rx * NA)[1];
            const float4 ay0 = reinterpret_cast<const float4*>(a.angles_y + ry * NA)[0], ay1 = reinterpret_cast<const float4*>(a.angles_y + ry * NA)[1];
            const float ax[NA] = {ax0.x, ax0.y, ax0.z, ax0.w, ax1.x, ax1.y, ax1.z, ax1.w};
            const float ay[NA] = {ay0.x, ay0.y, ay0.z, ay0.w, ay1.x, ay1.y, ay1.z, ay1.w};
            const unsigned long long dx = *reinterpret_cast<const unsigned long long*>(a.defined_x + rx * NA);
            const unsigned long long dy = *reinterpret_cast<const unsigned long long*>(a.defined_y + ry * NA);
            bool any_chi = false, all_in = true;
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const bool cmp = ((dx >> (8 * k)) & 0xff) && ((dy >> (8 * k)) & 0xff) && (k < 3 || same);
                if (!cmp) continue;
                float d = fabsf(ax[k] - ay[k]);
                if (d > PI_F) d = TWO_PI_F - d;
                if (k >= 4 && a.periodic[tx * 4 + (k - 4)] && d > HALF_PI_F) d = PI_F - d;
                d = fmaxf(d, 0.f);
                err[k] = d;
                esum[k] += (double)d;
                ecnt[k] += 1;
                const bool in = d <= tol;
                ewin[k] += in;
                if (k >= 4) {
                    any_chi = true;
                    all_in = all_in && in;
                }
            }
            n_chi += any_chi;
            n_correct += any_chi && all_in;

            if (same) {
                const float* X = spx + tid * RS;
                const float* Y = spy + tid * RS;
                const unsigned char* MX = smx + tid * MS;
                const unsigned char* MY = smy + tid * MS;
                const Frame fx = backbone_frame(X, MX), fy = backbone_frame(Y, MY);
                if (fx.ok && fy.ok) {
                    const unsigned char* sw = a.swap + tx * 4;
                    const int s0 = sw[0], s1 = sw[1], s2 = sw[2], s3 = sw[3];
                    const bool has0 = s0 != s1 && s0 < SL && s1 < SL, has1 = s2 != s3 && s2 < SL && s3 < SL;
                    bool can = has0 && MX[s0] && MX[s1] && MY[s0] && MY[s1];
                    if (has1) can = can && MX[s2] && MX[s3] && MY[s2] && MY[s3];
                    float plain = 0.f, alt = 0.f;
#pragma unroll
                    for (int s = 4; s < SL; ++s) {
                        if (!(MX[s] && MY[s])) continue;
                        int sx = s;
                        if (can) {
                            if (s == s0) sx = s1; else if (s == s1) sx = s0;
                            if (has1) { if (s == s2) sx = s3; else if (s == s3) sx = s2; }
                        }
                        float ly[3], lx[3], la[3];
                        to_local(fy, Y + s * 3, ly);
                        to_local(fx, X + s * 3, lx);
                        to_local(fx, X + sx * 3, la);
                        const float e0 = lx[0] - ly[0], e1 = lx[1] - ly[1], e2 = lx[2] - ly[2];
                        const float g0 = la[0] - ly[0], g1 = la[1] - ly[1], g2 = la[2] - ly[2];
                        plain += (e0 * e0 + e1 * e1) + e2 * e2;
                        alt += (g0 * g0 + g1 * g1) + g2 * g2;
                        ++sc_n;
                    }
                    swapped = can && alt < plain;
                    sc = swapped ? alt : plain;
                    sq_sum += (double)sc;
                    n_atoms_cmp += sc_n;
                }
            }
        }
        if (a.err) {
            const size_t o = p * N + n;
            reinterpret_cast<float4*>(a.err + o * NA)[0] = make_float4(err[0], err[1], err[2], err[3]);
            reinterpret_cast<float4*>(a.err + o * NA)[1] = make_float4(err[4], err[5], err[6], err[7]);
            a.sc_sq[o] = sc;
            a.sc_n[o] = sc_n;
            a.swapped[o] = swapped;
        }
    }

    __syncthreads();                                        // icnt is zeroed
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const double s = wave_tree_sum(esum[k]);
        if (lane == 0) dsum[wave][k] = s;
        if (ecnt[k]) atomicAdd(&icnt[k], ecnt[k]);
        if (ewin[k]) atomicAdd(&icnt[NA + k], ewin[k]);
    }
    {
        const double s = wave_tree_sum(sq_sum);
        if (lane == 0) dsum[wave][NA] = s;
    }
    if (n_chi) atomicAdd(&icnt[2 * NA], n_chi);
    if (n_correct) atomicAdd(&icnt[2 * NA + 1], n_correct);
    if (n_atoms_cmp) atomicAdd(&icnt[2 * NA + 2], n_atoms_cmp);
    __syncthreads();
    if (tid < NA) {
        a.err_sum[p * NA + tid] = dsum[0][tid] + dsum[1][tid];
        a.err_count[p * NA + tid] = icnt[tid];
        a.within[p * NA + tid] = icnt[NA + tid];
    }
    if (tid == 0) {
        const double s = dsum[0][NA] + dsum[1][NA];
        const int m = icnt[2 * NA + 2];
        a.res_with_chi[p] = icnt[2 * NA];
        a.res_correct[p] = icnt[2 * NA + 1];
        a.sc_sq_sum[p] = s;
        a.sc_atoms[p] = m;
        a.sc_rmsd[p] = m > 0 ? (float)sqrt(s / (double)m) : __builtin_nanf("");
    }
}

}  // namespace

extern "C" int pf_torsions_fwd(const pf_torsions_args* a, pf_stream_t stream) {
    if (!a || !a->pos || !a->atom_mask || !a->aa || !a->chi_atoms || !a->angles || !a->defined || a->B < 0 || a->N < 0 || a->n_atoms < SL)
        return PF_E_BADARG;
    if (a->B > 65535) return PF_E_TOOLARGE;
    if (a->B == 0 || a->N == 0) return 0;
    hipLaunchKernelGGL(torsions_kernel, dim3((unsigned)((a->N + TR - 1) / TR), (unsigned)a->B), dim3(NT), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}

extern "C" int pf_sidechain_compare_fwd(const pf_sidechain_compare_args* a, pf_stream_t stream) {
    if (!a || !a->pos_x || !a->pos_y || !a->mask_x || !a->mask_y || !a->aa_x || !a->aa_y || !a->angles_x || !a->angles_y || !a->defined_x ||
        !a->defined_y || !a->pairs || !a->periodic || !a->swap || !a->err_sum || !a->err_count || !a->within || !a->res_with_chi ||
        !a->res_correct || !a->sc_sq_sum || !a->sc_atoms || !a->sc_rmsd || a->Bx <= 0 || a->By <= 0 || a->N <= 0 || a->P < 0 ||
        a->n_atoms_x < SL || a->n_atoms_y < SL || !(a->correct_tol >= 0.f))
        return PF_E_BADARG;
    const int per_residue = (a->err != nullptr) + (a->sc_sq != nullptr) + (a->sc_n != nullptr) + (a->swapped != nullptr);
    if (per_residue != 0 && per_residue != 4) return PF_E_BADARG;
    if ((long long)a->N * NA > 0x7fffffffLL) return PF_E_TOOLARGE;
    if (a->P == 0) return 0;
    hipLaunchKernelGGL(sidechain_compare_kernel, dim3((unsigned)a->P), dim3(CT), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
