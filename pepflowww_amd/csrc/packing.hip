// pf_pack_sidechains_fwd -- rotamer side-chain packing of the movable residues of a batch of heavy-atom structures: every rotamer of a
// discrete table is built on the residue's own backbone, scored against the fixed environment with the pair function of
// pf_interface_energy_fwd, and one rotamer per residue is chosen by iterated conditional modes.  It is the step between
// reconstruct_sample_bb and pf_relax_fwd.  It is NOT SCWRL4 (which the reference's eval/run_scwrl4.py calls) and NOT Rosetta's packer:
// there is no Dunbrack library here (the default table is a staggered grid, geometry.rotamer_table), no hydrogens, no electrostatics, no
// graph decomposition and no fitted parameter; the energy is this package's own Vina-form pair energy.  It replaces those programs in
// role only, not in values.  Checked against the float64 restatement tests/pack_oracle.py and hand-computed cases.
//
// Conventions (tests/pack_oracle.py restates them in numpy float64):
//   Inputs    as pf_relax_fwd: pos [B,N,n_atoms,3], n_atoms >= 14, slots 0 .. min(n_atoms, 15) - 1 are read; atom_mask; aa;
//             residue_index; movable [B,N].  N <= 512.
//   Packed    a movable residue whose type is in 0..19 and whose N, CA and C are set in atom_mask.  Every other residue stays exactly
//             as given and is fixed environment.  packed [B,N].
//   Rotamers  rot_chi [21,max_rot,4] radians, rot_count [21] (clamped to 1 .. max_rot), rot_energy [21,max_rot]; max_rot <= 128.
//   Building  frame = construct_3d_basis(CA, C, N): e1 = u / (|u| + 1e-6), u = C - CA; e2 = v / (|v| + 1e-6), v = (N - CA) - (e1 . (N -
//             CA)) e1; e3 = e1 x e2; columns (e1, e2, e3), origin CA.  Then the chain of pf_full_atom_fwd: frame_k = frame_(k-1) o
//             (tab_rot[type, 3 + k] Rx(chi_k), tab_trans[type, 3 + k]), k = 1..4, frame_0 the backbone's.  The angle that turns frame_1
//             is chi_1 - eps: a rotamer's chi1 is the dihedral N-CA-CB-CG measured from the residue's REAL N, while the ideal groups turn
//             from where the ideal N (tab_pos[type, 0]) would be; eps is the signed angle about CA-CB from the real N to the ideal N,
//             taken in the backbone frame (atan2f of the two projections; 0 without a CB).  So geometry.torsion_angles gives the
//             row's chi back on any backbone; on an ideal backbone eps = 0 and this is pf_full_atom_fwd's chain bit for bit.  Rotamer atoms are the slots
//             5..13 that the type has (tab_mask) and whose tab_group is >= 4: at most 9.  CB (slot 4, group 0) is rebuilt once from
//             its ideal position in the backbone frame.  N, CA, C, O and slot 14 keep the input's bits and mask; slots 4..13 of the
//             output mask of a packed residue are the type's tab_mask; a slot the type lacks is written as 0.
//   Atoms     an input atom exists where atom_mask is set and radius [21,15] (the XS radii) has an entry for type row and slot; a
//             built atom exists where tab_mask has it.  Fixed atoms: every existing atom of an unpacked residue; N, CA, C, O, the
//             rebuilt CB and OXT of a packed one.
//   Energy    the pair function of pf_interface_energy_fwd (r < cutoff; d = r - R_i - R_j; gauss1, gauss2, repulsion, hydrophobic,
//             hbond; types bits), over
//               (a) a rotamer atom against every fixed atom of a residue of another residue_index;
//               (b) a rotamer atom against an atom of its own residue more than three bonds away (own_mask [21,15]: bit s' of (type,
//                   s), geometry.packing_pair_table; fixed slots and, each pair once, the rotamer atoms of a smaller slot);
//               (c) the rotamer atoms of two different packed residues of different residue_index.
//             Never evaluated: CYS SG against CYS SG (a disulfide is neither sought nor broken); across a peptide bond (the
//             partner's residue_index is the row's - 1) PRO CD against CA, C, O and PRO CG against C: fewer than four bonds apart
//             (an OXT on a residue that has a successor is not regarded).
//             E_self[m,r] = (a) + (b) + rot_energy[type, r];  E_pair = (c);  total = sum E_self of the chosen + sum over pairs m < m'.
//   Search    iterated conditional modes, deterministic.  Start: argmin_r E_self[m,r].  A sweep visits the packed residues in
//             ascending position; each takes the smallest r attaining the minimum of E_self[m,r] + sum_m' E_pair against the
//             current rotamers of the others.  It stops after a sweep that changed nothing, or after `sweeps`.  A local search.
//   Outputs   rotamer (-1: not packed), chi (the row's four values), n_rotamers, energy_self_best = E_self of the start,
//             energy_residue = E_self + half the residue's pair energy at the end, energy_trace [B,sweeps+1] float64 ([0]: the start;
//             sweeps not run repeat the last), sweeps_run, changed [B,sweeps] (rotamers changed per sweep; 0 for sweeps not run),
//             choice_trace [B,sweeps,N] optional (written at each visit; the caller fills it with -1 first).
//
// Arithmetic and summation order (fp32, -ffp-contract=off): a row atom keeps five term sums over its partners -- (a) column tiles
// ascending and the atoms of a tile ascending (residue, slot), then (b) slots ascending; (c) partner residues in ascending position, their
// atoms in ascending slot -- and only pairs inside the cutoff are added (adding nothing is exact, so culling does not show).  Row
// energy e = (((w0 t0 + w1 t1) + w2 t2) + w3 t3) + w4 t4.  E_self = ((e_0 + e_1) + ... + e_8) + rot_energy; a conditional energy =
// E_self + ((e_0 + e_1) + ... + e_8) of (c).  Total (float64): per packed residue E_self + the row energies of its pairs with later
// residues (partner ascending, slot ascending), thread t of 256 adds residues t, t + 256, ..., then a tree over the threads.  Every
// decision is an argmin under the total order (value, then index; NaN counts as +inf), so it does not depend on how lanes are paired.
// No atomics, one writer per output, nothing read back by the host: bit-identical from run to run and independent of the rest of the
// batch.
//   build_kernel   grid (N, B), 128 threads.  Thread 0 writes the residue's 15 environment atoms as float4 (x, y, z, radius; an absent
//                  one parked at x = -1e18, radius 0), their type bytes (bit 3: CYS SG) and its bounds (centre, extent over the fixed
//                  atoms).  Thread r < count builds rotamer r: 9 float4 (an absent one parked at x = +1e18).  The block's maximum of the
//                  atoms' distances from CA gives the rotamer bounds (centre CA, extent over all rotamers; -1: not packed).
//   self_kernel    the hot path.  Grid (tiles of 28 rotamers, N, B), 256 threads; thread t < 252 owns row (rotamer t / 9, atom t % 9).
//                  Environment tiles of 16 residues are staged in LDS as float4 plus type bytes plus residue_index, double-buffered;
//                  all lanes read the SAME column atom in a step (a broadcast, no bank conflict).  Wave 0 lists the tiles to visit:
//                  those with a residue whose centre is within (E + e_q + cutoff) of the row residue's CA, E and e_q the two extents.
//   search_kernel  one workgroup per sample.  The current rotamer atoms of its packed residues stay in LDS when there are at most 96
//                  of them, else they are read from the workspace.  The sweep loop, argmins, stop test, trace, totals and the output
//                  structure are all done here.  A pair of residues is looked at when their CAs are within (E + E' + cutoff).
#include "pack_dev.h"

namespace {

using namespace pack_dev;

constexpr int RT = 28, ROWS = RT * RA;                                  // rotamers and rows per workgroup of self_kernel
constexpr int LDS_RES = 96;                                             // packed residues whose current atoms fit in LDS

struct Work {
    float4* env;                    // [B,N,15]
    float4* rot;                    // [B,N,R,9]
    float4* ebound;                 // [B,N] centre, extent of the fixed atoms (-1: none)
    float4* rbound;                 // [B,N] CA, extent over all rotamers (-1: not packed)
    unsigned char* envflg;          // [B,N,16]
    float* eself;                   // [B,N,R]
};

__host__ __device__ inline Work carve(void* work, size_t rows, int R) {
    Work w;
    char* p = static_cast<char*>(work);
    w.env = reinterpret_cast<float4*>(p);                   p += rows * SL * sizeof(float4);
    w.rot = reinterpret_cast<float4*>(p);                   p += rows * (size_t)R * RA * sizeof(float4);
    w.ebound = reinterpret_cast<float4*>(p);                p += rows * sizeof(float4);
    w.rbound = reinterpret_cast<float4*>(p);                p += rows * sizeof(float4);
    w.envflg = reinterpret_cast<unsigned char*>(p);         p += rows * 16;
    w.eself = reinterpret_cast<float*>(p);
    return w;
}

constexpr long long BYTES_FIXED = SL * 16 + 16 + 16 + 16, BYTES_PER_ROT = RA * 16 + 4;     // per residue; per residue and rotamer

__global__ __launch_bounds__(MAXR) void build_kernel(pf_pack_args a, Work w) {
    __shared__ float wave_max[MAXR / 64];
    const int q = blockIdx.x, tid = threadIdx.x, A = a.n_atoms, R = a.max_rot;
    const size_t i = (size_t)blockIdx.y * a.N + q;
    const long long aa = a.aa[i];
    const int t = type_row(aa);
    const unsigned char* m = a.atom_mask + i * A;
    const float* p = a.pos + i * A * 3;
    const bool pk = a.movable[i] != 0 && aa >= 0 && aa <= 19 && m[0] != 0 && m[1] != 0 && m[2] != 0;

    Backbone F;
    backbone_frame(a, t, p, pk, F);

    if (tid == 0) {                                         // the environment atoms of this residue and their bounds
        float4 e[SL];
        unsigned char flg[SL];
        env_atoms(a, t, m, p, A, pk, F.cb, e, flg);
        for (int s = 0; s < SL; ++s) {
            w.env[i * SL + s] = e[s];
            w.envflg[i * 16 + s] = flg[s];
        }
        w.envflg[i * 16 + 15] = 0;
        w.ebound[i] = env_bound(e);
    }

    float ext = 0.f;
    if (pk && tid < rot_count(a, t)) {
        float4* dst = w.rot + (i * R + tid) * RA;
        for (int j = 0; j < RA; ++j) dst[j] = make_float4(FAR, 0.f, 0.f, 0.f);
        ext = build_rotamer(a, t, a.rot_chi + ((size_t)t * R + tid) * 4, F, [dst](int j, const float4& o) { dst[j] = o; });
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) ext = fmaxf(ext, __shfl_xor(ext, k));
    if ((tid & 63) == 0) wave_max[tid >> 6] = ext;
    __syncthreads();
    if (tid == 0) w.rbound[i] = make_float4(F.t[0], F.t[1], F.t[2], pk ? fmaxf(wave_max[0], wave_max[1]) : -1.f);
}

struct Tile {
    float4 at[TA];
    unsigned char flg[TA];
    int idx[TR];
};

struct Fetched {
    float4 at;
    unsigned char flg;
    int idx;
};

// thread t < 240: environment atom t of column tile ct of sample b; thread t < 16: residue t of it.  Addresses only for q < N.
__device__ __forceinline__ Fetched fetch_tile(const pf_pack_args& a, const Work& w, size_t b, int ct, int tid) {
    Fetched f;
    f.at = make_float4(-FAR, 0.f, 0.f, 0.f);
    f.flg = 0;
    f.idx = 0;
    if (tid < TA) {
        const int q = ct * TR + tid / SL, s = tid % SL;
        if (q < a.N) {
            f.at = w.env[(b * a.N + q) * SL + s];
            f.flg = w.envflg[(b * a.N + q) * 16 + s];
        }
    }
    if (tid < TR && ct * TR + tid < a.N) f.idx = a.residue_index[b * a.N + ct * TR + tid];
    return f;
}

__device__ __forceinline__ void commit_tile(Tile& t, const Fetched& f, int tid) {
    if (tid < TA) {
        t.at[tid] = f.at;
        t.flg[tid] = f.flg;
    }
    if (tid < TR) t.idx[tid] = f.idx;
}

__global__ __launch_bounds__(NT) void self_kernel(pf_pack_args a, Work w) {
    __shared__ Tile tile[2];
    __shared__ int list[MAX_TILES];
    __shared__ int n_list;
    __shared__ float erow[ROWS];
    const int N = a.N, R = a.max_rot, tid = threadIdx.x, q = blockIdx.y;
    const size_t b = blockIdx.z, i = b * N + q;
    const float4 C = w.rbound[i];
    if (C.w < 0.f) return;                                  // not packed (the whole workgroup)
    const int t = type_row(a.aa[i]), cnt = rot_count(a, t), r0 = blockIdx.x * RT;
    if (r0 >= cnt) return;
    const int n_tiles = (N + TR - 1) / TR;
    const float cutoff = a.cutoff, cut2 = cutoff * cutoff;
    const float4* ebound = w.ebound + b * N;

    const int r = r0 + tid / RA, j = tid % RA;
    const bool row = tid < ROWS && r < cnt;
    float4 P = make_float4(FAR, 0.f, 0.f, 0.f);
    if (row) P = w.rot[(i * R + r) * RA + j];
    const bool live = P.w > 0.f;
    const unsigned char fp = a.types[t * SL + S0 + j];
    const bool my_sg = t == a.cys && j == 0;
    const int pro_excl = t == a.pro ? (j == 1 ? 0xE : j == 0 ? 0x4 : 0) : 0;       // CD: CA, C, O; CG: C of the previous residue
    const long long my_idx = a.residue_index[i];

    if (tid < 64) {                                         // the column tiles to visit, ascending: wave 0, a tile per lane
        const bool keep = tid < n_tiles && tile_near(ebound, tid * TR, tid * TR + TR < N ? tid * TR + TR : N, C, cutoff);
        const unsigned long long bal = __ballot(keep);
        if (keep) list[__popcll(bal & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) n_list = __popcll(bal);
    }
    __syncthreads();
    const int n = n_list;

    float ts[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (n > 0) {
        commit_tile(tile[0], fetch_tile(a, w, b, list[0], tid), tid);
        __syncthreads();
    }
    for (int k = 0; k < n; ++k) {
        Fetched next;
        const bool more = k + 1 < n;
        if (more) next = fetch_tile(a, w, b, list[k + 1], tid);
        const Tile& T = tile[k & 1];
        for (int c = 0; c < TR; ++c) {
            const long long ci = T.idx[c];
            const int excl = ci == my_idx ? 0x7FFF : ci + 1 == my_idx ? pro_excl : 0;
#pragma unroll 5
            for (int s = 0; s < SL; ++s) {
                const float4 v = T.at[c * SL + s];
                const unsigned char f = T.flg[c * SL + s];
                if (!((excl >> s) & 1) && !(my_sg && (f & IS_SG))) pair_add(P, fp, v, f, cut2, ts);
            }
        }
        if (more) commit_tile(tile[(k + 1) & 1], next, tid);
        __syncthreads();
    }

    if (live) {                                             // (b): the own residue, slots ascending
        const int own = a.own_mask[t * SL + S0 + j];
        for (int s = 0; s < SL; ++s) {
            if (!((own >> s) & 1)) continue;
            const bool fixed = s < S0 || s == 14;
            const float4 v = fixed ? w.env[i * SL + s] : w.rot[(i * R + r) * RA + (s - S0)];
            if (v.w > 0.f) pair_add(P, fp, v, a.types[t * SL + s], cut2, ts);
        }
    }
    if (tid < ROWS) erow[tid] = live ? weighted(a, ts) : 0.f;
    __syncthreads();
    if (tid < RT && r0 + tid < cnt) {
        float e = erow[tid * RA];
        for (int k = 1; k < RA; ++k) e += erow[tid * RA + k];
        w.eself[i * R + r0 + tid] = e + a.rot_energy[(size_t)t * R + r0 + tid];
    }
}

struct SearchLds {
    float4 cur[LDS_RES * RA];       // the current rotamer atoms (when n_packed <= LDS_RES)
    float4 bound[MAXN];             // by packed position: CA, extent over all rotamers
    int q[MAXN];                    // by packed position: the residue
    int idx[MAXN];                  //                     its residue_index
    int rot[MAXN];                  //                     its current rotamer
    int rot_of_q[MAXN];             // by residue: its current rotamer, -1: not packed
    unsigned char type[MAXN], na[MAXN];
    unsigned char flg[MAXN * RA];
    float erow[MAXR * RA];
    float best_v[NT / 64];
    int best_i[NT / 64];
    double red[NT];
    int n_packed, n_changed;
};

__device__ __forceinline__ float4 cur_atom(const SearchLds& L, const Work& w, size_t row0, int R, bool fits, int p, int j) {
    return fits ? L.cur[p * RA + j] : w.rot[((row0 + L.q[p]) * R + L.rot[p]) * RA + j];
}

__device__ __forceinline__ bool near_pair(const SearchLds& L, int p, int p2, float cutoff) {
    const float4 u = L.bound[p], v = L.bound[p2];
    return L.idx[p] != L.idx[p2] && dist3(u, v) <= ((u.w + v.w) + cutoff) * CULL_SLACK + CULL_ABS;
}

// the five sums of the row atom P (flags fp, SG my_sg) of packed residue p over the current atoms of packed residue p2
__device__ __forceinline__ void pair_rows(const SearchLds& L, const Work& w, size_t row0, int R, bool fits, const float4& P,
                                          unsigned char fp, bool my_sg, int p2, float cut2, float ts[5]) {
    const int na = L.na[p2];
    for (int j2 = 0; j2 < na; ++j2) {
        const unsigned char f = L.flg[p2 * RA + j2];
        if (my_sg && (f & IS_SG)) continue;
        pair_add(P, fp, cur_atom(L, w, row0, R, fits, p2, j2), f, cut2, ts);
    }
}

// sum_j of the row energies of the current atoms of p against the residues p2 in [lo, hi) other than p, in fp32: partner ascending, slot ascending
__device__ float residue_pairs(const pf_pack_args& a, const SearchLds& L, const Work& w, size_t row0, bool fits, int p, int lo, int hi,
                               double* as_double) {
    const float cutoff = a.cutoff, cut2 = cutoff * cutoff;
    const int R = a.max_rot, na = L.na[p];
    float sum = 0.f;
    double dsum = 0.0;
    for (int p2 = lo; p2 < hi; ++p2) {
        if (p2 == p || !near_pair(L, p, p2, cutoff)) continue;
        for (int j = 0; j < na; ++j) {
            float ts[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            const unsigned char fp = L.flg[p * RA + j];
            pair_rows(L, w, row0, R, fits, cur_atom(L, w, row0, R, fits, p, j), fp, (fp & IS_SG) != 0, p2, cut2, ts);
            const float e = weighted(a, ts);
            sum += e;
            dsum += (double)e;
        }
    }
    if (as_double) *as_double = dsum;
    return sum;
}

__device__ double total_energy(const pf_pack_args& a, SearchLds& L, const Work& w, size_t row0, bool fits, int tid) {
    double acc = 0.0;
    const int n = L.n_packed;
    for (int p = tid; p < n; p += NT) {
        double pairs;
        residue_pairs(a, L, w, row0, fits, p, p + 1, n, &pairs);
        acc += (double)w.eself[(row0 + L.q[p]) * a.max_rot + L.rot[p]];
        acc += pairs;
    }
    return block_sum<NT>(acc, L.red, tid);
}

__global__ __launch_bounds__(NT) void search_kernel(pf_pack_args a, Work w) {
    __shared__ SearchLds L;
    const int N = a.N, R = a.max_rot, tid = threadIdx.x, S = a.sweeps;
    const size_t b = blockIdx.x, row0 = b * N;
    const float cutoff = a.cutoff, cut2 = cutoff * cutoff;

    if (tid == 0) {                                         // the packed residues, ascending
        int n = 0;
        for (int q = 0; q < N; ++q)
            if (w.rbound[row0 + q].w >= 0.f) L.q[n++] = q;
        L.n_packed = n;
    }
    for (int q = tid; q < N; q += NT) L.rot_of_q[q] = -1;
    __syncthreads();
    const int n = L.n_packed;
    const bool fits = n <= LDS_RES;
    for (int p = tid; p < n; p += NT) {                     // the start: argmin_r E_self
        const size_t i = row0 + L.q[p];
        const int t = type_row(a.aa[i]), cnt = rot_count(a, t);
        int na = 0;
        for (int j = 0; j < RA; ++j) {
            const int g = a.tab_group[t * 14 + S0 + j];
            const bool has = a.tab_mask[t * SL + S0 + j] && g >= 4 && g <= 7;
            na += has;                                      // (the atoms of a type fill its slots from the front)
            L.flg[p * RA + j] = w.envflg[i * 16 + S0 + j];
        }
        L.type[p] = (unsigned char)t;
        L.na[p] = (unsigned char)na;
        L.idx[p] = a.residue_index[i];
        L.bound[p] = w.rbound[i];
        float bv = no_nan(w.eself[i * R]);
        int bi = 0;
        for (int r = 1; r < cnt; ++r) {
            const float v = no_nan(w.eself[i * R + r]);
            if (better(v, r, bv, bi)) {
                bv = v;
                bi = r;
            }
        }
        L.rot[p] = bi;
        a.energy_self_best[i] = w.eself[i * R + bi];
    }
    __syncthreads();
    if (fits)
        for (int k = tid; k < n * RA; k += NT) L.cur[k] = w.rot[((row0 + L.q[k / RA]) * R + L.rot[k / RA]) * RA + k % RA];
    __syncthreads();

    double* trace = a.energy_trace + b * (S + 1);
    double e_now = total_energy(a, L, w, row0, fits, tid);
    if (tid == 0) trace[0] = e_now;
    int run = 0;
    for (int sweep = 0; sweep < S; ++sweep) {
        if (tid == 0) L.n_changed = 0;
        for (int p = 0; p < n; ++p) {
            const int q = L.q[p];
            const size_t i = row0 + q;
            const int cnt = rot_count(a, L.type[p]), na = L.na[p];
            for (int row = tid; row < cnt * RA; row += NT) {
                const int r = row / RA, j = row % RA;
                float e = 0.f;
                if (j < na) {
                    const float4 P = w.rot[(i * R + r) * RA + j];
                    const unsigned char fp = L.flg[p * RA + j];
                    float ts[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
                    for (int p2 = 0; p2 < n; ++p2)
                        if (p2 != p && near_pair(L, p, p2, cutoff)) pair_rows(L, w, row0, R, fits, P, fp, (fp & IS_SG) != 0, p2, cut2, ts);
                    e = weighted(a, ts);
                }
                L.erow[row] = e;
            }
            __syncthreads();
            float v = INFINITY;
            int vi = 0x7fffffff;
            if (tid < cnt) {                                // cnt <= 128: waves 0 and 1
                float e = L.erow[tid * RA];
                for (int k = 1; k < RA; ++k) e += L.erow[tid * RA + k];
                v = no_nan(w.eself[i * R + tid] + e);
                vi = tid;
            }
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) {
                const float v2 = __shfl_xor(v, k);
                const int i2 = __shfl_xor(vi, k);
                if (better(v2, i2, v, vi)) {
                    v = v2;
                    vi = i2;
                }
            }
            if ((tid & 63) == 0) {
                L.best_v[tid >> 6] = v;
                L.best_i[tid >> 6] = vi;
            }
            __syncthreads();
            const int best = better(L.best_v[1], L.best_i[1], L.best_v[0], L.best_i[0]) ? L.best_i[1] : L.best_i[0];
            const bool moved = best != L.rot[p];
            __syncthreads();                                // every thread has read rot[p] and best_*
            if (moved) {
                if (fits && tid < RA) L.cur[p * RA + tid] = w.rot[(i * R + best) * RA + tid];
                if (tid == 0) {
                    L.rot[p] = best;
                    L.n_changed += 1;
                }
            }
            if (tid == 0 && a.choice_trace) a.choice_trace[(b * S + sweep) * N + q] = best;
            __syncthreads();
        }
        e_now = total_energy(a, L, w, row0, fits, tid);
        const int changed = L.n_changed;
        if (tid == 0) {
            trace[sweep + 1] = e_now;
            a.changed[b * S + sweep] = changed;
        }
        run = sweep + 1;
        __syncthreads();                                    // n_changed is reset at the top of the next sweep
        if (changed == 0) break;
    }
    if (tid == 0) {
        a.sweeps_run[b] = run;
        for (int s = run; s < S; ++s) {
            trace[s + 1] = e_now;
            a.changed[b * S + s] = 0;
        }
    }

    for (int p = tid; p < n; p += NT) {
        const size_t i = row0 + L.q[p];
        const float pairs = residue_pairs(a, L, w, row0, fits, p, 0, n, nullptr);
        a.energy_residue[i] = w.eself[i * R + L.rot[p]] + 0.5f * pairs;
        L.rot_of_q[L.q[p]] = L.rot[p];
    }
    __syncthreads();
    const int A = a.n_atoms;
    for (int q = tid; q < N; q += NT) {
        const size_t i = row0 + q;
        const int r = L.rot_of_q[q], t = type_row(a.aa[i]);
        a.packed[i] = r >= 0;
        a.rotamer[i] = r;
        a.n_rotamers[i] = r >= 0 ? rot_count(a, t) : 0;
        if (r < 0) {
            a.energy_self_best[i] = 0.f;
            a.energy_residue[i] = 0.f;
        }
        for (int k = 0; k < 4; ++k) a.chi[i * 4 + k] = r >= 0 ? a.rot_chi[((size_t)t * R + r) * 4 + k] : 0.f;
    }
    for (int k = tid; k < N * SL; k += NT) {
        const int q = k / SL, s = k % SL;
        const size_t i = row0 + q;
        const int r = L.rot_of_q[q], t = type_row(a.aa[i]);
        float x[3] = {0.f, 0.f, 0.f};
        unsigned char mk = 0;
        if (r < 0 || s < 4 || s == 14) {                    // the input's bits
            if (s < A) {
                const float* p = a.pos + (i * A + s) * 3;
                x[0] = p[0]; x[1] = p[1]; x[2] = p[2];
                mk = a.atom_mask[i * A + s];
            }
        } else {
            mk = a.tab_mask[t * SL + s];
            const float4 v = s == 4 ? w.env[i * SL + 4] : w.rot[(i * R + r) * RA + (s - S0)];
            if (mk && v.w > 0.f) { x[0] = v.x; x[1] = v.y; x[2] = v.z; }
        }
        float* o = a.pos_out + (i * SL + s) * 3;
        o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
        a.mask_out[i * SL + s] = mk;
    }
}

__host__ inline bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" int pf_pack_work_bytes(int B, int N, int max_rot) {
    if (B < 0 || N < 0 || N > PF_PACK_MAX_N || max_rot < 1 || max_rot > PF_PACK_MAX_ROT) return -1;
    const long long bytes = (long long)B * N * (BYTES_FIXED + BYTES_PER_ROT * max_rot);
    return bytes > 0x7fffffffLL ? -1 : (int)bytes;
}

extern "C" int pf_pack_sidechains_fwd(const pf_pack_args* a, pf_stream_t stream) {
    if (!a || !a->pos || !a->atom_mask || !a->aa || !a->residue_index || !a->movable || !a->radius || !a->types || !a->own_mask ||
        !a->tab_rot || !a->tab_trans || !a->tab_group || !a->tab_pos || !a->tab_mask || !a->rot_chi || !a->rot_count ||
        !a->rot_energy || !a->work || !a->pos_out || !a->mask_out || !a->packed || !a->rotamer || !a->chi || !a->n_rotamers ||
        !a->energy_self_best || !a->energy_residue || !a->energy_trace || !a->sweeps_run || (!a->changed && a->sweeps > 0) || a->B < 0 || a->N < 0 ||
        a->n_atoms < SL - 1 || a->max_rot < 1 || a->sweeps < 0 || !(a->cutoff > 0.f) || !(a->cutoff < 1e6f) || !finite_f(a->w_gauss1) ||
        !finite_f(a->w_gauss2) || !finite_f(a->w_repulsion) || !finite_f(a->w_hydrophobic) || !finite_f(a->w_hbond))
        return PF_E_BADARG;
    if (a->N > PF_PACK_MAX_N || a->max_rot > PF_PACK_MAX_ROT || a->B > 65535) return PF_E_TOOLARGE;
    if (pf_pack_work_bytes(a->B, a->N, a->max_rot) < 0) return PF_E_TOOLARGE;
    if (a->B == 0 || a->N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const Work w = carve(a->work, (size_t)a->B * a->N, a->max_rot);
    hipLaunchKernelGGL(build_kernel, dim3((unsigned)a->N, (unsigned)a->B), dim3(MAXR), 0, st, *a, w);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(self_kernel, dim3((unsigned)((a->max_rot + RT - 1) / RT), (unsigned)a->N, (unsigned)a->B), dim3(NT), 0, st, *a, w);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(search_kernel, dim3((unsigned)a->B), dim3(NT), 0, st, *a, w);
    PF_CHECK_LAUNCH();
    return 0;
}
