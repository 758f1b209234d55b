// pf_interface_energy_fwd -- an empirical interface energy between the groups of a batch of heavy-atom structures (a peptide and its
// receptor): the functional form of AutoDock Vina's scoring function (Trott & Olson, J. Comput. Chem. 31, 2010) over heavy atoms, no
// hydrogens.  Written from the publication; checked against the float64 restatement tests/energy_oracle.py and hand-computed cases.
// It is NOT checked against the Vina program and is not Vina's output (no ligand preparation, no torsion tree, no hydrogens), and it
// is not Rosetta's dG_separated.
//
// Conventions (tests/energy_oracle.py restates them in numpy float64):
//   Atoms     slots 0 .. min(n_atoms, 15) - 1 of pos [B,N,n_atoms,3] in the package's heavy-atom order (slot 14 is OXT), n_atoms >= 14.
//             An atom takes part where atom_mask is set and radius [21,15] has a non-zero entry for the package's residue type (a type
//             outside 0..19 reads row 20: N, CA, C, O) and the slot.
//   Pairs     (i, j) is evaluated when the residues' group bytes differ, both atoms take part and r_ij < cutoff (8 A).  Nothing inside
//             a group is ever evaluated.
//   Surface   d = r_ij - R_i - R_j with the XS radii by element: C 1.9, N 1.8, O 1.7, S 2.0 A.
//   Terms     0 gauss1       exp(-(d / 0.5)^2)                                           every pair
//             1 gauss2       exp(-((d - 3) / 2)^2)                                       every pair
//             2 repulsion    d^2 if d < 0, else 0                                        every pair
//             3 hydrophobic  1 for d <= 0.5, linear to 0 at d >= 1.5                      both atoms hydrophobic
//             4 hbond        1 for d <= -0.7, linear to 0 at d >= 0                       one a donor, the other an acceptor
//   Typing    types [21,15] bytes: bit 0 hydrophobic, bit 1 donor, bit 2 acceptor (geometry.interface_type_table: from chemistry
//             without hydrogens; both ring nitrogens of histidine are donor and acceptor, the tautomer being unknown).
//   Outputs   per row atom: terms_atom [B,N,15,5] fp32 = the unweighted sums over its partners; pairs_atom, hbond_pairs_atom,
//             hydrophobic_pairs_atom [B,N,15] int32 = partners inside the cutoff, with hbond > 0, with hydrophobic > 0.  Per row
//             residue: terms_residue [B,N,5] = the fp32 sum over the slots in slot order; energy_residue [B,N] =
//             (((w0 t0 + w1 t1) + w2 t2) + w3 t3) + w4 t4 in fp32.  Each pair shows in both of its rows: a structure's total is half
//             the sum over all rows (taken in float64 by the caller).
//   query     [B,N]: only atoms of query residues are rows; every participating atom is still a partner.  A participating atom that
//             is not a row has the three counts -1 and zero terms, as in pf_sasa_fwd; its residue's sums are zero.
//
// Two launches, no atomics, nothing pair-sized: every output has one writer, every sum a fixed order (column tiles ascending, the atoms
// of a tile ascending, the slots of a residue ascending), so the results are bit-identical from run to run and depend neither on the
// rest of the batch nor on its order.
//   bounds_kernel  a thread per residue: work [B,N,4] = (centre, extent): the coordinates of its CA (or of its first participating atom)
//                  and the largest distance of a participating atom from it (-1: no atom).
//   energy_kernel  grid (row tiles of 16 residues, B), 256 threads; thread t < 240 owns row atom (t / 15, t % 15) and walks every atom
//                  of every kept column tile.  Column tiles are staged in LDS as float4 (x, y, z, R) plus one flag byte per atom and
//                  one group byte per residue, double-buffered.  All lanes of a wave read the SAME column atom in a step: a broadcast,
//                  which has no bank conflict whatever the stride.  The radius stays a bit-exact fp32 in w and the three flag bits
//                  ride in a byte beside it: packing them into w's low mantissa bits would move R by up to 8 ulp, which is the whole
//                  positional budget of the test.  An atom that does not take part is parked at x = +1e18 (row) / -1e18 (column), so
//                  the cutoff test removes it and no lane branches on a mask.  Wave 0 builds the list of column tiles to visit, a
//                  tile per lane: those holding a residue of another group than the row tile's that lies within (E + e_q + cutoff) of
//                  the row tile's centre, E and e_q being the row tile's and the residue's extents (a superset of the tiles with a
//                  pair inside the cutoff).  A thread keeps five fp32 sums and three int32 counts; only pairs inside the cutoff are
//                  added (adding nothing is exact), in ascending column order.  The 15 slots of a residue are summed in slot order
//                  through LDS by one thread per residue (stride 15 dwords between residues: odd, no bank conflict).
//
// Exponential: expf, not __expf.  HIP's math API documents expf with a maximum error of 1 ulp; __expf (v_exp_f32 on x * log2 e) has
// no documented bound in ulp of the result, and its argument rounding grows with |x| up to 85 here.  The test's error model uses the
// 1 ulp.  Only pairs inside the cutoff reach it.
#include "common.h"
#include "../../include/pepflow_hip.h"
#include "eval_dev.h"

namespace {

constexpr int TR = 16, SL = PF_INTERFACE_ENERGY_SLOTS, TA = TR * SL;    // residues per tile, slots per residue, atoms per tile
constexpr int NT = 256;
constexpr int MAX_TILES = PF_INTERFACE_ENERGY_MAX_N / TR;
constexpr int NTERM = 5;
constexpr float FAR = 1e18f;
constexpr float CULL_SLACK = 1.0001f;
constexpr unsigned char HYDROPHOBIC = 1, DONOR = 2, ACCEPTOR = 4;

struct Tile {
    float4 a[TA];                   // x, y, z, R
    unsigned char flg[TA];          // type bits
    unsigned char grp[TR];
};

struct Fetched {
    float4 a;
    unsigned char flg, grp, exists;
};

__device__ __forceinline__ float dist3(const float4& p, const float4& q) {
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

__global__ __launch_bounds__(256) void bounds_kernel(pf_interface_energy_args a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.B * a.N) return;
    const int A = a.n_atoms, S = A < SL ? A : SL;
    const float* p = a.pos + i * A * 3;
    const unsigned char* m = a.atom_mask + i * A;
    const float* rad = a.radius + type_row(a.aa[i]) * SL;
    int c = -1;                                             // slot 1 (CA) if it takes part, else the first slot that does
    if (m[1] && rad[1] > 0.f) c = 1;
    for (int s = 0; s < S && c < 0; ++s)
        if (m[s] && rad[s] > 0.f) c = s;
    float4 w = make_float4(0.f, 0.f, 0.f, -1.f);
    if (c >= 0) {
        w = make_float4(p[3 * c], p[3 * c + 1], p[3 * c + 2], 0.f);
        for (int s = 0; s < S; ++s)
            if (m[s] && rad[s] > 0.f) w.w = fmaxf(w.w, dist3(make_float4(p[3 * s], p[3 * s + 1], p[3 * s + 2], 0.f), w));
    }
    reinterpret_cast<float4*>(a.work)[i] = w;
}

// thread t < 240: atom t of tile ct of structure b (one that does not take part: x = far); thread t < 16: residue t of it.  Every
// address is formed only for q < N, s < n_atoms.
__device__ __forceinline__ Fetched fetch_tile(const pf_interface_energy_args& a, size_t b, int ct, int tid, float far) {
    Fetched f;
    f.a = make_float4(far, 0.f, 0.f, 0.f);
    f.flg = f.grp = f.exists = 0;
    const int N = a.N, A = a.n_atoms;
    if (tid < TA) {
        const int q = ct * TR + tid / SL, s = tid % SL;
        if (q < N && s < A) {
            const size_t r = b * N + q;
            const int tr = type_row(a.aa[r]);
            const float rad = a.radius[tr * SL + s];
            if (a.atom_mask[r * A + s] != 0 && rad > 0.f) {
                const float* p = a.pos + (r * A + s) * 3;
                f.a = make_float4(p[0], p[1], p[2], rad);
                f.flg = a.types[tr * SL + s];
                f.exists = 1;
            }
        }
    }
    if (tid < TR) {
        const int q = ct * TR + tid;
        if (q < N) f.grp = a.group[b * N + q];
    }
    return f;
}

__device__ __forceinline__ void commit_tile(Tile& t, const Fetched& f, int tid) {
    if (tid < TA) {
        t.a[tid] = f.a;
        t.flg[tid] = f.flg;
    }
    if (tid < TR) t.grp[tid] = f.grp;
}

__global__ __launch_bounds__(NT) void energy_kernel(pf_interface_energy_args a) {
    __shared__ Tile tile[2];
    __shared__ unsigned char row_grp[TR];
    __shared__ int list[MAX_TILES];
    __shared__ int n_list;
    __shared__ float red[NTERM][TA];
    const int N = a.N, tid = threadIdx.x;
    const size_t b = blockIdx.y;
    const int rt = blockIdx.x, n_tiles = (N + TR - 1) / TR;
    const int r0 = rt * TR, r1 = r0 + TR < N ? r0 + TR : N;
    const float cutoff = a.cutoff, cut2 = cutoff * cutoff;
    const unsigned char* query = a.query ? a.query + b * N : nullptr;
    const unsigned char* group = a.group + b * N;
    const float4* work = reinterpret_cast<const float4*>(a.work) + b * N;

    // the thread's row atom: parked unless it takes part and its residue is a row
    Fetched me = fetch_tile(a, b, rt, tid, FAR);
    const int rr = tid < TA ? tid / SL : 0;
    const bool is_row = me.exists && (!query || query[r0 + rr] != 0);
    if (!is_row) me.a = make_float4(FAR, 0.f, 0.f, 0.f);
    if (tid < TR) row_grp[tid] = me.grp;

    // the column tiles to visit, ascending: wave 0, a tile per lane
    if (tid < 64) {
        int rc = -1, best = 2 * TR, lo = 256, hi = -1;      // the row residue nearest the tile's middle; the rows' group bytes
        for (int r = r0; r < r1; ++r) {
            const int off = 2 * (r - r0) - (TR - 1), dist = off < 0 ? -off : off;
            if (work[r].w >= 0.f && (!query || query[r])) {
                lo = min(lo, (int)group[r]);
                hi = max(hi, (int)group[r]);
                if (dist < best) {
                    best = dist;
                    rc = r;
                }
            }
        }
        bool keep = false;
        if (rc >= 0 && tid < n_tiles) {                     // (rc is the same in every lane)
            const float4 C = work[rc];
            float E = 0.f;
            for (int r = r0; r < r1; ++r) {
                const float4 w = work[r];
                if (w.w >= 0.f && (!query || query[r])) E = fmaxf(E, dist3(w, C) + w.w);
            }
            const int q1 = tid * TR + TR < N ? tid * TR + TR : N;
            for (int q = tid * TR; q < q1; ++q) {
                const float4 w = work[q];
                const bool other = lo != hi || (int)group[q] != lo;
                keep = keep || (w.w >= 0.f && other && dist3(w, C) <= ((E + w.w) + cutoff) * CULL_SLACK);
            }
        }
        const unsigned long long bal = __ballot(keep);
        if (keep) list[__popcll(bal & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) n_list = __popcll(bal);
    }
    __syncthreads();
    const int cnt = n_list;
    const unsigned char my_grp = row_grp[rr];
    const float4 P = me.a;
    const bool my_h = (me.flg & HYDROPHOBIC) != 0, my_d = (me.flg & DONOR) != 0, my_a = (me.flg & ACCEPTOR) != 0;

    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f, t4 = 0.f;
    int n_in = 0, n_hb = 0, n_hp = 0;

    if (cnt > 0) {
        commit_tile(tile[0], fetch_tile(a, b, list[0], tid, -FAR), tid);
        __syncthreads();
    }
    for (int k = 0; k < cnt; ++k) {
        Fetched next;
        const bool more = k + 1 < cnt;
        if (more) next = fetch_tile(a, b, list[k + 1], tid, -FAR);
        const Tile& T = tile[k & 1];
        for (int c = 0; c < TR; ++c) {
            const bool other = T.grp[c] != my_grp;
#pragma unroll 5
            for (int s = 0; s < SL; ++s) {
                const float4 v = T.a[c * SL + s];
                const unsigned char f = T.flg[c * SL + s];
                const float dx = P.x - v.x, dy = P.y - v.y, dz = P.z - v.z;
                const float r2 = (dx * dx + dy * dy) + dz * dz;
                if (other && r2 < cut2) {
                    const float d = sqrtf(r2) - (P.w + v.w);
                    const float g1 = d * 2.f, g2 = (d - 3.f) * 0.5f;
                    t0 += expf(-(g1 * g1));
                    t1 += expf(-(g2 * g2));
                    t2 += d < 0.f ? d * d : 0.f;
                    const bool hp = my_h && (f & HYDROPHOBIC);
                    const bool hb = (my_d && (f & ACCEPTOR)) || (my_a && (f & DONOR));
                    const float vhp = !hp ? 0.f : d <= 0.5f ? 1.f : d >= 1.5f ? 0.f : 1.5f - d;
                    const float vhb = !hb ? 0.f : d <= -0.7f ? 1.f : d >= 0.f ? 0.f : d * (-1.f / 0.7f);
                    t3 += vhp;
                    t4 += vhb;
                    n_in += 1;
                    n_hp += vhp > 0.f;
                    n_hb += vhb > 0.f;
                }
            }
        }
        if (more) commit_tile(tile[(k + 1) & 1], next, tid);
        __syncthreads();
    }

    if (tid < TA) {
        red[0][tid] = t0;
        red[1][tid] = t1;
        red[2][tid] = t2;
        red[3][tid] = t3;
        red[4][tid] = t4;
        const int r = r0 + rr, s = tid % SL;
        if (r < N) {
            const size_t o = (b * N + r) * SL + s;
            const int skipped = me.exists && !is_row ? -1 : 0;
            float* ta = a.terms_atom + o * NTERM;
            ta[0] = t0; ta[1] = t1; ta[2] = t2; ta[3] = t3; ta[4] = t4;
            a.pairs_atom[o] = skipped ? -1 : n_in;
            a.hbond_pairs_atom[o] = skipped ? -1 : n_hb;
            a.hydrophobic_pairs_atom[o] = skipped ? -1 : n_hp;
        }
    }
    __syncthreads();
    if (tid < TR && r0 + tid < N) {
        float s[NTERM];
        for (int k = 0; k < NTERM; ++k) {
            s[k] = 0.f;
            for (int t = 0; t < SL; ++t) s[k] += red[k][tid * SL + t];
        }
        const size_t o = b * N + r0 + tid;
        for (int k = 0; k < NTERM; ++k) a.terms_residue[o * NTERM + k] = s[k];
        a.energy_residue[o] = (((a.w_gauss1 * s[0] + a.w_gauss2 * s[1]) + a.w_repulsion * s[2]) + a.w_hydrophobic * s[3]) + a.w_hbond * s[4];
    }
}

__host__ inline bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" int pf_interface_energy_fwd(const pf_interface_energy_args* a, pf_stream_t stream) {
    if (!a || !a->pos || !a->atom_mask || !a->aa || !a->group || !a->radius || !a->types || !a->work || !a->terms_atom ||
        !a->terms_residue || !a->energy_residue || !a->pairs_atom || !a->hbond_pairs_atom || !a->hydrophobic_pairs_atom || a->B < 0 ||
        a->N < 0 || a->n_atoms < SL - 1 || !(a->cutoff > 0.f) || !(a->cutoff < 1e6f) || !finite_f(a->w_gauss1) ||
        !finite_f(a->w_gauss2) || !finite_f(a->w_repulsion) || !finite_f(a->w_hydrophobic) || !finite_f(a->w_hbond))
        return PF_E_BADARG;
    if (a->N > PF_INTERFACE_ENERGY_MAX_N || a->B > 65535) return PF_E_TOOLARGE;
    if (a->B == 0 || a->N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)a->B * a->N;
    hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, *a);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(energy_kernel, dim3((unsigned)((a->N + TR - 1) / TR), (unsigned)a->B), dim3(NT), 0, st, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
