// pf_sasa_fwd -- solvent-accessible surface area of a batch of heavy-atom structures by the method of Shrake & Rupley (J. Mol. Biol.
// 79, 1973): every atom carries P test points on the sphere of its radius plus the probe's, and its accessible area is the share of
// those points that lie inside no other atom's sphere.  With `group` the same pass also gives every group's surface on its own, so
// the area buried between a peptide and its receptor is one call.
//
// Conventions (tests/sasa_oracle.py restates them in numpy):
//   Atoms     slots 0 .. min(n_atoms, 15) - 1 of pos [B,N,n_atoms,3] in the package's heavy-atom order (slot 14 is OXT), n_atoms >= 14.
//             An atom exists where atom_mask is set and radius [21,15] has a non-zero entry for the package's residue type (a type
//             outside 0..19 reads row 20) and the slot: Bondi's C 1.7, N 1.55, O 1.52, S 1.8.  No hydrogens.
//   Points    points [P,3] fp32 unit vectors u_k (geometry.sphere_points: a golden spiral), 1 <= P <= 1024, read through a pointer.
//   Test      R_a = radius_a + probe_radius, rounded to fp32.  Point k of atom a is buried by atom b when b != a, b is in the same
//             structure and exists (atoms of a's own residue count), and |d + R_a u_k|^2 < R_b^2 with d = x_a - x_b formed first, in
//             fp32 (a correctly rounded difference of the fp32 coordinates: the result does not depend on where the structure sits in
//             space).  The rest is fp32: t = d + R_a * u_k per component (a rounded product, a rounded sum), then
//             fma(t_z, t_z, fma(t_y, t_y, t_x * t_x)) < R_b * R_b.
//             Coincident atoms follow from the rule: the larger buries the smaller.
//   Outputs   count [B,N,15] int32 = accessible points; sasa_atom = 4 pi R_a^2 count / P, evaluated in fp64 and rounded to fp32;
//             sasa_residue [B,N] = the fp32 sum over the slots in slot order; sasa_total [B] = the sum of sasa_atom over the structure
//             in fp64 (a fixed tree), rounded to fp32.  An absent atom has count 0 and area 0.
//   group     [B,N], zero / non-zero as in pf_violations_fwd.  The *_own outputs are the same quantities with only the atoms of
//             residues of a's own group as partners; both come from one pass (a point carries two flags), and count_own >= count.
//   query     [B,N]: only atoms of query residues are evaluated; every existing atom is still a partner.  An existing atom that is
//             not evaluated has count -1 and area 0 and does not enter the sums.
//
// Three launches, no atomics, nothing pair-, point- or neighbour-list-sized in global memory: every output has one writer and every
// sum a fixed order, and a point's state is an OR over its partners, which no order changes; so the results are bit-identical from
// run to run and do not depend on the rest of the batch.
//   bounds_kernel  a thread per residue: work [B,N,4] = (centre, padded extent), centre = the coordinates of its CA (or of its first
//                  existing atom), padded extent = max over its atoms of |x - centre| + R (-1: no atom).  The centre is an atom's own
//                  coordinates, so every length below is formed from correctly rounded differences, whatever the coordinates' size.
//   sasa_kernel    grid (row tiles of 16 residues, B), 256 threads (512 for N > 256).  The row tile's evaluated residues get a
//                  bounding sphere (C, E) in the same way; a residue q can hold a partner only if |c_q - C| < E + e_q, and the atoms
//                  of the residues that pass are compacted (existing atoms only, ballot + per-wave counts) into LDS as
//                  (x, y, z, R_b) plus a 16-bit id with the group bit.  The LDS is sized for N * 15 atoms, which is why N <= 512: the
//                  stage cannot overflow.  Then one wave per atom at a time, a wave owning whole residues: 64 staged atoms per step
//                  are tested against |d| < R_a + R_b (with slack: a superset), the hits compacted by ballot into the wave's LDS list
//                  as (d, R_b^2) plus an own-group byte; whenever the next 64 might not fit the list (128 entries) it is walked and
//                  emptied, so a crowded atom only takes more walks.  A walk reads one entry per step (the same LDS word for all
//                  lanes) and tests it against the lane's ceil(P / 64) points, held in registers as R_a u_k, OR-ing two bit masks;
//                  it ends early once every point of every lane is buried under both flags.  Counts are summed over the wave with
//                  wave_sum; lane 0 writes the atom's and the residue's outputs.
//   total_kernel   one block per sample: the fp64 sums.
#include "common.h"
#include "../../include/pepflow_hip.h"
#include "eval_dev.h"

namespace {

constexpr int TR = 16, SL = PF_SASA_SLOTS;
constexpr int LCAP = 128;                   // entries of a wave's neighbour list (>= 64: one step's hits always fit an empty list)
constexpr int NT_MAX = 512;
constexpr float NEAR_SLACK = 1.0001f, CULL_SLACK = 1.0001f;
constexpr unsigned short ID_MASK = 0x7fff, ID_GROUP = 0x8000;

__host__ __device__ inline size_t sasa_lds_bytes(int N, int nw) {
    const size_t cap = (size_t)N * SL;
    return 16 * cap + 16 * (size_t)nw * LCAP + 64 + 2 * ((cap + 1) & ~(size_t)1) + 2 * PF_SASA_MAX_N + (size_t)nw * LCAP;
}

__global__ __launch_bounds__(256) void bounds_kernel(pf_sasa_args a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.B * a.N) return;
    const int A = a.n_atoms, S = A < SL ? A : SL;
    const float* p = a.pos + i * A * 3;
    const unsigned char* m = a.atom_mask + i * A;
    const float* rad = a.radius + type_row(a.aa[i]) * SL;
    int c = -1;                                             // slot 1 (CA) if it exists, else the first existing slot
    if (m[1] && rad[1] > 0.f) c = 1;
    for (int s = 0; s < S && c < 0; ++s)
        if (m[s] && rad[s] > 0.f) c = s;
    float4 w = make_float4(0.f, 0.f, 0.f, -1.f);
    if (c >= 0) {
        w = make_float4(p[3 * c], p[3 * c + 1], p[3 * c + 2], 0.f);
        for (int s = 0; s < S; ++s)
            if (m[s] && rad[s] > 0.f) {
                const float dx = p[3 * s] - w.x, dy = p[3 * s + 1] - w.y, dz = p[3 * s + 2] - w.z;
                w.w = fmaxf(w.w, sqrtf((dx * dx + dy * dy) + dz * dz) + (rad[s] + a.probe_radius));
            }
    }
    reinterpret_cast<float4*>(a.work)[i] = w;
}

// exclusive offset of this thread's flag among the block's set flags, in thread order, and their number; two barriers
__device__ __forceinline__ int block_offsets(bool flag, int* wcnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const unsigned long long bal = __ballot(flag);
    __syncthreads();                                        // the previous round's readers are done with wcnt
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int off = __popcll(bal & ((1ull << lane) - 1ull));
    total = 0;
    for (int w = 0; w < nw; ++w) {
        const int c = wcnt[w];
        if (w < wave) off += c;
        total += c;
    }
    return off;
}

// the wave's list against the lane's points; true once every point of every lane is buried under both flags
template <int KP>
__device__ __forceinline__ bool walk(const float4* nb, const unsigned char* nb_own, int n, const float (&px)[KP], const float (&py)[KP],
                                     const float (&pz)[KP], unsigned& bur, unsigned& own) {
    constexpr unsigned full = (1u << KP) - 1u;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the list's writes (this wave's own) have landed
    bool done = false;
    for (int i = 0; i < n; ++i) {
        const float4 e = nb[i];
        const unsigned om = nb_own[i] ? 0xffffffffu : 0u;
        unsigned hit = 0;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const float tx = e.x + px[k], ty = e.y + py[k], tz = e.z + pz[k];
            hit |= (__builtin_fmaf(tz, tz, __builtin_fmaf(ty, ty, tx * tx)) < e.w ? 1u : 0u) << k;
        }
        bur |= hit;
        own |= hit & om;
        if (__ballot((bur & own & full) != full) == 0ull) {
            done = true;
            break;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the reads are done before the list is refilled
    return done;
}

template <int KP>
__global__ __launch_bounds__(NT_MAX) void sasa_kernel(pf_sasa_args a) {
    extern __shared__ __align__(16) char sasa_lds[];
    const int N = a.N, A = a.n_atoms, S = A < SL ? A : SL, P = a.n_points;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = blockDim.x, nw = nt >> 6;
    const size_t b = blockIdx.y;
    const int r0 = blockIdx.x * TR, r1 = r0 + TR < N ? r0 + TR : N;
    const float probe = a.probe_radius;
    constexpr unsigned full = (1u << KP) - 1u;

    const size_t cap = (size_t)N * SL;
    float4* at = reinterpret_cast<float4*>(sasa_lds);                           // [cap] staged partners (x, y, z, R_b)
    float4* nb_all = at + cap;                                                  // [nw][LCAP] (d, R_b^2)
    int* wcnt = reinterpret_cast<int*>(nb_all + (size_t)nw * LCAP);             // [16]
    unsigned short* id = reinterpret_cast<unsigned short*>(wcnt + 16);          // [cap] residue * 15 + slot, bit 15: group
    unsigned short* rlist = id + ((cap + 1) & ~(size_t)1);                      // [512] residues that pass the cull
    unsigned char* nbo_all = reinterpret_cast<unsigned char*>(rlist + PF_SASA_MAX_N);   // [nw][LCAP] partner of the own group
    float4* nb = nb_all + (size_t)wave * LCAP;
    unsigned char* nbo = nbo_all + (size_t)wave * LCAP;

    const float4* work = reinterpret_cast<const float4*>(a.work) + b * N;
    const unsigned char* query = a.query ? a.query + b * N : nullptr;
    const unsigned char* group = a.group ? a.group + b * N : nullptr;

    // the bounding sphere of the tile's evaluated residues, about the centre of the one nearest to the tile's middle
    int rc = -1, best = 2 * TR;
    for (int r = r0; r < r1; ++r) {
        const int off = 2 * (r - r0) - (TR - 1), dist = off < 0 ? -off : off;
        if (work[r].w >= 0.f && (!query || query[r]) && dist < best) {
            best = dist;
            rc = r;
        }
    }
    int ns = 0;
    if (rc >= 0) {                                          // (the same in every thread of the block)
        const float4 C = work[rc];
        float E = 0.f;
        for (int r = r0; r < r1; ++r) {
            const float4 w = work[r];
            if (w.w >= 0.f && (!query || query[r])) {
                const float dx = w.x - C.x, dy = w.y - C.y, dz = w.z - C.z;
                E = fmaxf(E, sqrtf((dx * dx + dy * dy) + dz * dz) + w.w);
            }
        }
        // residues that can hold a partner, in ascending order
        int nres = 0;
        for (int q0 = 0; q0 < N; q0 += nt) {
            const int q = q0 + tid;
            bool keep = false;
            if (q < N) {
                const float4 w = work[q];
                const float dx = w.x - C.x, dy = w.y - C.y, dz = w.z - C.z;
                keep = w.w >= 0.f && sqrtf((dx * dx + dy * dy) + dz * dz) <= (E + w.w) * CULL_SLACK;
            }
            int total;
            const int off = block_offsets(keep, wcnt, total);
            if (keep) rlist[nres + off] = (unsigned short)q;
            nres += total;
        }
        __syncthreads();
        // their existing atoms
        const int ncand = nres * S;
        for (int i0 = 0; i0 < ncand; i0 += nt) {
            const int i = i0 + tid;
            bool ok = false;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            unsigned short iv = 0;
            if (i < ncand) {
                const int q = rlist[i / S], s = i % S;
                const size_t r = b * N + q;
                const float rad = a.radius[type_row(a.aa[r]) * SL + s];
                if (a.atom_mask[r * A + s] && rad > 0.f) {
                    const float* p = a.pos + (r * A + s) * 3;
                    ok = true;
                    v = make_float4(p[0], p[1], p[2], rad + probe);
                    iv = (unsigned short)((q * SL + s) | (group && group[q] ? ID_GROUP : 0));
                }
            }
            int total;
            const int off = block_offsets(ok, wcnt, total);
            if (ok) {
                at[ns + off] = v;
                id[ns + off] = iv;
            }
            ns += total;
        }
        __syncthreads();
    }

    // the lane's points: k * 64 + lane, k < KP; those beyond P count as buried from the start
    float ux[KP], uy[KP], uz[KP];
    unsigned pad = 0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const int j = k * 64 + lane;
        const bool in = j < P;
        const float* u = a.points + 3 * (size_t)(in ? j : 0);
        ux[k] = in ? u[0] : 0.f;
        uy[k] = in ? u[1] : 0.f;
        uz[k] = in ? u[2] : 0.f;
        if (!in) pad |= 1u << k;
    }

    const bool has_own = a.count_own != nullptr;
    for (int r = r0 + wave; r < r1; r += nw) {
        const size_t row = b * N + r;
        const bool evaluated = !query || query[r];
        const float* radrow = a.radius + type_row(a.aa[row]) * SL;
        const unsigned ga = group && group[r] ? 1u : 0u;
        float res = 0.f, res_own = 0.f;
        for (int s = 0; s < SL; ++s) {
            float rad = 0.f;
            if (s < S && a.atom_mask[row * A + s]) rad = radrow[s];
            const bool exists = __builtin_amdgcn_readfirstlane(rad > 0.f ? 1 : 0) != 0;
            int cnt = 0, cnt_own = 0;
            float area = 0.f, area_own = 0.f;
            if (exists && !evaluated) {
                cnt = cnt_own = -1;
            } else if (exists) {
                const float* p = a.pos + (row * A + s) * 3;
                const float xa = p[0], ya = p[1], za = p[2], Ra = rad + probe;
                const unsigned ida = (unsigned)(r * SL + s);
                float px[KP], py[KP], pz[KP];
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    px[k] = Ra * ux[k];
                    py[k] = Ra * uy[k];
                    pz[k] = Ra * uz[k];
                }
                unsigned bur = pad, own = pad;
                int nl = 0;
                bool done = false;
                for (int j0 = 0; j0 < ns && !done; j0 += 64) {
                    const int j = j0 + lane;
                    const bool valid = j < ns;
                    const int jj = valid ? j : ns - 1;
                    const float4 c = at[jj];
                    const unsigned ci = id[jj];
                    const float dx = xa - c.x, dy = ya - c.y, dz = za - c.z;
                    const float lim = Ra + c.w;
                    const bool near = valid && (ci & ID_MASK) != ida && (dx * dx + dy * dy) + dz * dz <= lim * lim * NEAR_SLACK;
                    const unsigned long long bal = __ballot(near);
                    const int n = __popcll(bal);
                    if (nl + n > LCAP) {                    // the list may not hold them: walk it and go on with an empty one
                        done = walk<KP>(nb, nbo, nl, px, py, pz, bur, own);
                        nl = 0;
                    }
                    if (near) {
                        const int o = nl + __popcll(bal & ((1ull << lane) - 1ull));
                        nb[o] = make_float4(dx, dy, dz, c.w * c.w);
                        nbo[o] = (unsigned char)(!has_own || (ci >> 15) == ga);
                    }
                    nl += n;
                }
                if (!done) walk<KP>(nb, nbo, nl, px, py, pz, bur, own);
                cnt = (int)wave_sum((float)__popc(~bur & full));
                cnt_own = (int)wave_sum((float)__popc(~own & full));
                const double sphere = 4.0 * 3.14159265358979323846 * (double)Ra * (double)Ra / (double)P;
                area = (float)(sphere * (double)cnt);
                area_own = (float)(sphere * (double)cnt_own);
            }
            res += area;
            res_own += area_own;
            if (lane == 0) {
                const size_t o = row * SL + s;
                a.count[o] = cnt;
                a.sasa_atom[o] = area;
                if (has_own) {
                    a.count_own[o] = cnt_own;
                    a.sasa_atom_own[o] = area_own;
                }
            }
        }
        if (lane == 0) {
            a.sasa_residue[row] = res;
            if (has_own) a.sasa_residue_own[row] = res_own;
        }
    }
}

__global__ __launch_bounds__(256) void total_kernel(pf_sasa_args a) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x, na = (size_t)a.N * SL;
    double s = 0.0, s_own = 0.0;
    for (size_t i = tid; i < na; i += 256) {
        s += (double)a.sasa_atom[b * na + i];
        if (a.sasa_atom_own) s_own += (double)a.sasa_atom_own[b * na + i];
    }
    s = block_sum<256>(s, red, tid);
    s_own = block_sum<256>(s_own, red, tid);
    if (tid == 0) {
        a.sasa_total[b] = (float)s;
        if (a.sasa_total_own) a.sasa_total_own[b] = (float)s_own;
    }
}

template <int KP>
int launch(const pf_sasa_args& a, hipStream_t stream) {
    const int nt = a.N > 256 ? NT_MAX : 256;
    const size_t lds = sasa_lds_bytes(a.N, nt / 64);
    static PfOncePerDevice attr;
    if (lds > 64 * 1024 && attr.first())
        (void)hipFuncSetAttribute((const void*)sasa_kernel<KP>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(sasa_kernel<KP>, dim3((unsigned)((a.N + TR - 1) / TR), (unsigned)a.B), dim3(nt), lds, stream, a);
    PF_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int pf_sasa_fwd(const pf_sasa_args* a, pf_stream_t stream) {
    if (!a || !a->pos || !a->atom_mask || !a->aa || !a->radius || !a->points || !a->work || !a->count || !a->sasa_atom ||
        !a->sasa_residue || !a->sasa_total || a->B < 0 || a->N < 0 || a->n_atoms < SL - 1 || a->n_points < 1 ||
        a->n_points > PF_SASA_MAX_POINTS || !(a->probe_radius >= 0.f) || !(a->probe_radius < 1e6f))
        return PF_E_BADARG;
    const int n_own = (a->count_own != nullptr) + (a->sasa_atom_own != nullptr) + (a->sasa_residue_own != nullptr) +
                      (a->sasa_total_own != nullptr);
    if ((n_own != 0 && n_own != 4) || (n_own && !a->group)) return PF_E_BADARG;
    if (a->N > PF_SASA_MAX_N || a->B > 65535) return PF_E_TOOLARGE;
    if (a->B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (a->N > 0) {
        const size_t rows = (size_t)a->B * a->N;
        hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, *a);
        PF_CHECK_LAUNCH();
        const int kp = (a->n_points + 63) / 64;
        int rc;
        if (kp <= 1) rc = launch<1>(*a, st);
        else if (kp <= 2) rc = launch<2>(*a, st);
        else if (kp <= 4) rc = launch<4>(*a, st);
        else if (kp <= 8) rc = launch<8>(*a, st);
        else if (kp <= 15) rc = launch<15>(*a, st);
        else rc = launch<16>(*a, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(total_kernel, dim3((unsigned)a->B), dim3(256), 0, st, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
