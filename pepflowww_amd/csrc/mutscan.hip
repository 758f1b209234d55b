// pf_mutation_scan_fwd -- point-mutation scanning of chosen residues of a batch of heavy-atom structures: at every scanned residue,
// every rotamer of each of the 20 residue types is built on the residue's own backbone and scored against the structure as it stands,
// and the best rotamer of each type is reported.  energy[q,t] - energy[q,aa[q]] is the quantity of an alanine scan (t = ALA) or of a
// position scan (all t).  It stands where the reference's evaluation calls FoldX (eval/foldx.py: AlaScan, PositionScan) or Rosetta, in
// role only: it is NOT FoldX and NOT Rosetta.  The energy is packing.hip's E_self (this package's Vina-form pair energy plus the rotamer
// table's energy): no solvation, no electrostatics, no entropy, no backbone movement, no repacking of neighbours; defaults untuned.
// Checked against the float64 restatement tests/scan_oracle.py and, bit for bit, against pf_pack_sidechains_fwd on mutated inputs.
//
// Definition (conventions as packing.hip; tests/scan_oracle.py restates them in numpy float64):
//   Inputs    as pf_pack_sidechains_fwd, with positions [B,N] in place of movable; candidates [B,N,20] bytes, optional (null: every
//             type); group [B,N] bytes, optional.  N <= 512.
//   Scanned   a residue q where positions is set, whose type aa[q] is in 0..19 and whose N, CA and C are in atom_mask.  scanned [B,N].
//   Evaluated (q, t), t in 0..19, where q is scanned and t is a candidate or t = aa[q] (the wild type is always evaluated).
//   E[q,t,r]  packing.hip's E_self of rotamer r of type t on q's backbone; every other residue is fixed environment exactly as given,
//             side chains included, other scanned residues too: single-point mutants, neighbours are not repacked.
//     rows    the rotamer atoms of type t (slots 5..13 that tab_mask has with tab_group >= 4), built by packing's frame chain with the
//             chi1 offset from the real N (pack_dev.h: backbone_frame, build_rotamer).
//     own     the residue's fixed atoms are the given N, CA, C, O and slot 14 and CB rebuilt from type t's ideal position; their radii,
//             type bits and own_mask are type t's, not aa[q]'s.
//     terms   (a) rows against every existing atom of a residue of another residue_index (an input atom exists where atom_mask is set
//             and radius has an entry for the residue's own type row and slot); (b) own-residue pairs more than three bonds apart
//             (own_mask[t]); plus rot_energy[t,r].
//     never   CYS SG (t = CYS) against a CYS SG; across a peptide bond (partner's residue_index = q's - 1), t = PRO: CD against CA,
//             C, O and CG against C.
//   Choice    energy[q,t] = min_r E[q,t,r], rotamer[q,t] the smallest r attaining it; NaN counts as +inf under (value, index).
//   Outputs   scanned [B,N]; per (q, t): energy (+inf where not evaluated), rotamer (-1), n_rotamers (0), chi [4] (the chosen row; 0),
//             energy_interface (+inf): the part of (a) of the chosen rotamer whose partner residue has a group byte different from
//             q's -- the same five sums in the same order over those partners only, weighted and added over the rows in the same way
//             (no table energy); 0 without group.
//   Consequences: ALA and GLY have no rotamer atom, so their energy is the table's (0 by default) and energy[q,ALA] - energy[q,aa[q]]
//             is minus the contribution of the side chain beyond CB.  Differences in the backbone (PRO's N, GLY's missing CB) do not show.
//
// Arithmetic and summation order (fp32, -ffp-contract=off) are packing.hip's: a row atom's five term sums run over (a) column tiles
// ascending and the atoms of a tile ascending (residue, slot), then (b) slots ascending, adding only pairs inside the cutoff (so culling
// does not show); row energy e = (((w0 t0 + w1 t1) + w2 t2) + w3 t3) + w4 t4; E = ((e_0 + e_1) + ... + e_8) + rot_energy (a slot the
// type lacks adds 0).  energy[q,t] has the bits of pf_pack_sidechains_fwd's energy_self_best on the input with aa[q] := t and q alone
// movable.  No atomics, one writer per output, nothing read back by the host: bit-identical from run to run and independent of the
// rest of the batch, of the other positions and of the other candidates.
//   env_kernel   a thread per residue: its 15 environment atoms as float4 (x, y, z, radius; absent: x = -1e18, radius 0), their type
//                bytes, its bounds (centre, extent) and `scanned`.  The workspace: 272 bytes per residue, nothing per type or rotamer.
//   scan_kernel  grid (20 types, N, B), 256 threads; a workgroup whose (q, t) is not evaluated writes the fill values and exits.
//                Thread r < count builds rotamer r in registers and leaves its <= 9 atoms in LDS (18 KiB for 128 rotamers): no
//                rotamer ever reaches global memory.  Rows are compacted to the atoms the type has, (rotamer, atom) -> thread, 256 rows
//                a pass (SER: 3 rows, GLN: 432), so a pass is not spent on slots a type lacks.  A pass walks the culled environment
//                tiles of 16 residues through LDS, double-buffered, every lane reading the same column atom in a step (a broadcast);
//                wave 0 lists the tiles once per workgroup (bounds as self_kernel: the extent over all rotamers of the type).  Row
//                energies go to LDS; thread r < count adds its nine and the argmin is a butterfly under (value, index).
#include "pack_dev.h"

namespace {

using namespace pack_dev;

constexpr int NTYPES = PF_MUTATION_SCAN_TYPES;
constexpr int ENV_NT = 128;
constexpr long long BYTES_RES = SL * 16 + 16 + 16;                      // env, ebound, envflg

struct Work {
    float4* env;                    // [B,N,15]
    float4* ebound;                 // [B,N] centre, extent of the residue's atoms (-1: none)
    unsigned char* envflg;          // [B,N,16]
};

__host__ __device__ inline Work carve(void* work, size_t rows) {
    Work w;
    char* p = static_cast<char*>(work);
    w.env = reinterpret_cast<float4*>(p);                   p += rows * SL * sizeof(float4);
    w.ebound = reinterpret_cast<float4*>(p);                p += rows * sizeof(float4);
    w.envflg = reinterpret_cast<unsigned char*>(p);
    return w;
}

__device__ __forceinline__ bool is_scanned(const pf_mutation_scan_args& a, size_t i) {
    const long long aa = a.aa[i];
    const unsigned char* m = a.atom_mask + i * a.n_atoms;
    return a.positions[i] != 0 && aa >= 0 && aa <= 19 && m[0] != 0 && m[1] != 0 && m[2] != 0;
}

__global__ __launch_bounds__(ENV_NT) void env_kernel(pf_mutation_scan_args a, Work w) {
    const size_t i = (size_t)blockIdx.x * ENV_NT + threadIdx.x;
    if (i >= (size_t)a.B * a.N) return;
    const int A = a.n_atoms, t = type_row(a.aa[i]);
    const float none[3] = {0.f, 0.f, 0.f};
    float4 e[SL];
    unsigned char flg[SL];
    env_atoms(a, t, a.atom_mask + i * A, a.pos + i * A * 3, A, false, none, e, flg);
    for (int s = 0; s < SL; ++s) {
        w.env[i * SL + s] = e[s];
        w.envflg[i * 16 + s] = flg[s];
    }
    w.envflg[i * 16 + 15] = 0;
    w.ebound[i] = env_bound(e);
    a.scanned[i] = is_scanned(a, i);
}

struct Tile {
    float4 at[TA];
    unsigned char flg[TA];
    int idx[TR];
    unsigned char grp[TR];
};

struct Fetched {
    float4 at;
    unsigned char flg, grp;
    int idx;
};

// thread t < 240: environment atom t of column tile ct of sample b; thread t < 16: residue t of it.  Addresses only for q < N.
__device__ __forceinline__ Fetched fetch_tile(const pf_mutation_scan_args& a, const Work& w, size_t b, int ct, int tid) {
    Fetched f;
    f.at = make_float4(-FAR, 0.f, 0.f, 0.f);
    f.flg = 0;
    f.grp = 0;
    f.idx = 0;
    if (tid < TA) {
        const int q = ct * TR + tid / SL, s = tid % SL;
        if (q < a.N) {
            f.at = w.env[(b * a.N + q) * SL + s];
            f.flg = w.envflg[(b * a.N + q) * 16 + s];
        }
    }
    if (tid < TR && ct * TR + tid < a.N) {
        f.idx = a.residue_index[b * a.N + ct * TR + tid];
        if (a.group) f.grp = a.group[b * a.N + ct * TR + tid];
    }
    return f;
}

__device__ __forceinline__ void commit_tile(Tile& t, const Fetched& f, int tid) {
    if (tid < TA) {
        t.at[tid] = f.at;
        t.flg[tid] = f.flg;
    }
    if (tid < TR) {
        t.idx[tid] = f.idx;
        t.grp[tid] = f.grp;
    }
}

struct ScanLds {
    Tile tile[2];
    float4 rot[MAXR * RA];          // every rotamer of the type, built here
    float4 own[SL];                 // the residue's fixed atoms as type t has them
    float erow[MAXR * RA];          // row energies: (a) + (b)
    float irow[MAXR * RA];          //               the part of (a) across groups
    int list[MAX_TILES];
    int n_list;
    int live[RA], na;               // the rotamer atoms the type has, ascending
    float wave_max[NT / 64];
    float best_v[2];
    int best_i[2];
};

// seqdesign.hip's self_kernel is this kernel's twin (the same rows, tiles, sums and order) and promises its bits: a change here belongs there.
__global__ __launch_bounds__(NT) void scan_kernel(pf_mutation_scan_args a, Work w) {
    __shared__ ScanLds L;
    const int N = a.N, R = a.max_rot, A = a.n_atoms, tid = threadIdx.x, t = blockIdx.x, q = blockIdx.y;
    const size_t b = blockIdx.z, i = b * N + q, o = i * NTYPES + t;
    const bool asked = is_scanned(a, i) && (a.aa[i] == t || !a.candidates || a.candidates[o] != 0);
    if (!asked) {                                           // (the whole workgroup)
        if (tid == 0) {
            a.energy[o] = INFINITY;
            a.energy_interface[o] = INFINITY;
            a.rotamer[o] = -1;
            a.n_rotamers[o] = 0;
        }
        if (tid < 4) a.chi[o * 4 + tid] = 0.f;
        return;
    }
    const int cnt = rot_count(a, t), n_tiles = (N + TR - 1) / TR;
    const float cutoff = a.cutoff, cut2 = cutoff * cutoff;
    const unsigned char* m = a.atom_mask + i * A;
    const float* p = a.pos + i * A * 3;

    Backbone F;
    backbone_frame(a, t, p, true, F);
    if (tid == 0) {                                         // the own residue's fixed atoms, as type t
        float4 e[SL];
        unsigned char flg[SL];
        env_atoms(a, t, m, p, A, true, F.cb, e, flg);
        for (int s = 0; s < SL; ++s) L.own[s] = e[s];
    }
    float ext = 0.f;
    if (tid < cnt) {
        float4* dst = L.rot + tid * RA;
        for (int j = 0; j < RA; ++j) dst[j] = make_float4(FAR, 0.f, 0.f, 0.f);
        ext = build_rotamer(a, t, a.rot_chi + ((size_t)t * R + tid) * 4, F, [dst](int j, const float4& v) { dst[j] = v; });
    }
    for (int k = tid; k < cnt * RA; k += NT) L.erow[k] = L.irow[k] = 0.f;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) ext = fmaxf(ext, __shfl_xor(ext, k));
    if ((tid & 63) == 0) L.wave_max[tid >> 6] = ext;
    __syncthreads();
    const float4 C = make_float4(F.t[0], F.t[1], F.t[2], fmaxf(L.wave_max[0], L.wave_max[1]));     // cnt <= 128: waves 0 and 1

    if (tid < 64) {                                         // the column tiles to visit, ascending: wave 0, a tile per lane
        const bool keep = tid < n_tiles && tile_near(w.ebound + b * N, tid * TR, tid * TR + TR < N ? tid * TR + TR : N, C, cutoff);
        const unsigned long long bal = __ballot(keep);
        if (keep) L.list[__popcll(bal & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) {
            L.n_list = __popcll(bal);
            int na = 0;                                     // a row is an atom that exists and has a radius (rotamer 0 shows it)
            for (int j = 0; j < RA; ++j)
                if (L.rot[j].w > 0.f) L.live[na++] = j;
            L.na = na;
        }
    }
    __syncthreads();
    const int n = L.n_list, na = L.na, rows = cnt * na;
    const long long my_idx = a.residue_index[i];
    const unsigned char my_grp = a.group ? a.group[i] : 0;

    for (int row0 = 0; row0 < rows; row0 += NT) {
        const bool has = row0 + tid < rows;
        const int r = has ? (row0 + tid) / na : 0, j = has ? L.live[(row0 + tid) % na] : 0;
        const float4 P = has ? L.rot[r * RA + j] : make_float4(FAR, 0.f, 0.f, 0.f);
        const unsigned char fp = a.types[t * SL + S0 + j];
        const bool my_sg = t == a.cys && j == 0;
        const int pro_excl = t == a.pro ? (j == 1 ? 0xE : j == 0 ? 0x4 : 0) : 0;   // CD: CA, C, O; CG: C of the previous residue
        float ts[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, ti[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (n > 0) {
            commit_tile(L.tile[0], fetch_tile(a, w, b, L.list[0], tid), tid);
            __syncthreads();
        }
        for (int k = 0; k < n; ++k) {                       // (a)
            Fetched next;
            const bool more = k + 1 < n;
            if (more) next = fetch_tile(a, w, b, L.list[k + 1], tid);
            const Tile& T = L.tile[k & 1];
            for (int c = 0; c < TR; ++c) {
                const long long ci = T.idx[c];
                const int excl = ci == my_idx ? 0x7FFF : ci + 1 == my_idx ? pro_excl : 0;
                const bool across = T.grp[c] != my_grp;
#pragma unroll 5
                for (int s = 0; s < SL; ++s) {
                    const float4 v = T.at[c * SL + s];
                    const unsigned char f = T.flg[c * SL + s];
                    float term[5];
                    if (!((excl >> s) & 1) && !(my_sg && (f & IS_SG)) && pair_terms(P, fp, v, f, cut2, term)) {
#pragma unroll
                        for (int x = 0; x < 5; ++x) {
                            ts[x] += term[x];
                            if (across) ti[x] += term[x];
                        }
                    }
                }
            }
            if (more) commit_tile(L.tile[(k + 1) & 1], next, tid);
            __syncthreads();
        }
        if (has) {
            const float ei = weighted(a, ti);
            const int own = a.own_mask[t * SL + S0 + j];    // (b): the own residue, slots ascending
            for (int s = 0; s < SL; ++s) {
                if (!((own >> s) & 1)) continue;
                const float4 v = (s < S0 || s == 14) ? L.own[s] : L.rot[r * RA + (s - S0)];
                if (v.w > 0.f) pair_add(P, fp, v, a.types[t * SL + s], cut2, ts);
            }
            L.erow[r * RA + j] = weighted(a, ts);
            L.irow[r * RA + j] = ei;
        }
    }
    __syncthreads();

    float e = 0.f, v = INFINITY;
    int vi = 0x7fffffff;
    if (tid < cnt) {                                        // cnt <= 128: waves 0 and 1
        e = L.erow[tid * RA];
        for (int k = 1; k < RA; ++k) e += L.erow[tid * RA + k];
        e = e + a.rot_energy[(size_t)t * R + tid];
        v = no_nan(e);
        vi = tid;
    }
    if (tid < 128) {
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
    }
    __syncthreads();
    const int best = better(L.best_v[1], L.best_i[1], L.best_v[0], L.best_i[0]) ? L.best_i[1] : L.best_i[0];
    if (tid == best) {                                      // one writer: the thread that holds E of the chosen rotamer
        float ei = L.irow[best * RA];
        for (int k = 1; k < RA; ++k) ei += L.irow[best * RA + k];
        a.energy[o] = e;
        a.energy_interface[o] = ei;
        a.rotamer[o] = best;
        a.n_rotamers[o] = cnt;
        for (int k = 0; k < 4; ++k) a.chi[o * 4 + k] = a.rot_chi[((size_t)t * R + best) * 4 + k];
    }
}

__host__ inline bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" int pf_mutation_scan_work_bytes(int B, int N) {
    if (B < 0 || N < 0 || N > PF_PACK_MAX_N) return -1;
    const long long bytes = (long long)B * N * BYTES_RES;
    return bytes > 0x7fffffffLL ? -1 : (int)bytes;
}

extern "C" int pf_mutation_scan_fwd(const pf_mutation_scan_args* a, pf_stream_t stream) {
    if (!a || !a->pos || !a->atom_mask || !a->aa || !a->residue_index || !a->positions || !a->radius || !a->types || !a->own_mask ||
        !a->tab_rot || !a->tab_trans || !a->tab_group || !a->tab_pos || !a->tab_mask || !a->rot_chi || !a->rot_count ||
        !a->rot_energy || !a->work || !a->scanned || !a->energy || !a->rotamer || !a->n_rotamers || !a->chi || !a->energy_interface ||
        a->B < 0 || a->N < 0 || a->n_atoms < SL - 1 || a->max_rot < 1 || !(a->cutoff > 0.f) || !(a->cutoff < 1e6f) ||
        !finite_f(a->w_gauss1) || !finite_f(a->w_gauss2) || !finite_f(a->w_repulsion) || !finite_f(a->w_hydrophobic) ||
        !finite_f(a->w_hbond))
        return PF_E_BADARG;
    if (a->N > PF_PACK_MAX_N || a->max_rot > PF_PACK_MAX_ROT || a->B > 65535) return PF_E_TOOLARGE;
    if (pf_mutation_scan_work_bytes(a->B, a->N) < 0) return PF_E_TOOLARGE;
    if (a->B == 0 || a->N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)a->B * a->N;
    const Work w = carve(a->work, rows);
    hipLaunchKernelGGL(env_kernel, dim3((unsigned)((rows + ENV_NT - 1) / ENV_NT)), dim3(ENV_NT), 0, st, *a, w);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_kernel, dim3(NTYPES, (unsigned)a->N, (unsigned)a->B), dim3(NT), 0, st, *a, w);
    PF_CHECK_LAUNCH();
    return 0;
}
