// pf_sequence_design_fwd -- fixed-backbone sequence design of chosen residues of a batch of heavy-atom structures: the residue TYPE and
// the rotamer of every designed residue are chosen together by iterated conditional modes over all candidate (type, rotamer) pairs,
// with the backbone and every other residue fixed.  It closes the loop sample -> design -> pack -> relax -> score on the device and
// stands where the reference's eval/run_mpnn.py runs ProteinMPNN over the peptide chain of backbone-only samples, in role only: it is
// NOT ProteinMPNN and NOT Rosetta fixbb.  The energy is this package's Vina-form pair energy (the pair function of
// pf_interface_energy_fwd) plus the rotamer table's energy plus an optional per-type reference energy the caller supplies: no
// solvation, no electrostatics, no entropy, no learned prior, no backbone movement; WITHOUT REFERENCE ENERGIES IT FAVOURS LARGE SIDE
// CHAINS (more atoms, more attractive pairs); a deterministic local search, not the global minimum; defaults untuned, no fitted
// parameter.  Checked against the float64 restatement tests/seqdesign_oracle.py and, bit for bit, against pf_mutation_scan_fwd.
//
// Definition (conventions as packing.hip and mutscan.hip; tests/seqdesign_oracle.py restates them in numpy float64):
//   Inputs    as pf_pack_sidechains_fwd, with designed [B,N] in place of movable; candidates [B,N,20] bytes, optional; ref_energy [20],
//             optional.  N <= 512.
//   Designed  a residue q where designed is set, whose type aa[q] is in 0..19 and whose N, CA and C are in atom_mask.  Its candidates
//             are the types whose candidates byte is set (null: all 20); an empty set is {aa[q]} (so the residue is simply repacked).
//             A sample with more than max_res (<= 64) designed residues gets status 1 and comes back as if nothing were designed;
//             this is decided on the device.
//   State     every designed residue m has a current (t_m, r_m).  Its current atoms: N, CA, C, O and slot 14 as given, CB rebuilt from
//             type t_m (absent for GLY), the rotamer atoms of (t_m, r_m); radii, type bits and own_mask are row t_m's.  Its frame atoms:
//             the same without the rotamer atoms.
//   Energy    the pair function and the never-evaluated pairs of packing.hip: CYS SG against CYS SG; across a peptide bond (the
//             partner's residue_index is the row's - 1) PRO CD against CA, C, O and PRO CG against C, wherever a PRO rotamer atom is
//             the row.
//     E_self[m,t,r]  mutscan.hip's E[q,t,r] over the residues that are NOT designed (rows against every existing atom of every
//                    non-designed residue of another residue_index, own-residue pairs of type t, rot_energy[t,r]), then + ref_energy[t]
//                    (the add is skipped when ref_energy is null).
//     P[m,t,r]       the rotamer atoms of (t, r) against all current atoms of every other designed residue of another residue_index.
//     F[m,t]         the current rotamer atoms of every other designed residue (of another residue_index) against the frame atoms of m
//                    under type t.  packing.hip has no such term: there a partner's CB and type bits never change; here they do, and
//                    with F every difference of two conditional energies is a difference of the total, so the search is monotone.
//     conditional(m,t,r) = E_self + P + F.
//     total          sum_m E_self(m) + sum_m sum_(m' != m) rot(m) against frame(m') + sum_(m < m') rot(m) against rot(m').
//   Search    iterated conditional modes, deterministic.  Start: per residue the argmin of E_self over its candidate (t, r).  A sweep
//             visits the designed residues in ascending position; each takes the argmin of the conditional over its candidate (t, r).
//             It stops after a sweep that changed nothing, or after `sweeps`.  Every argmin is under the total order (value, then t,
//             then r); NaN counts as +inf.  Then one profile pass: profile[q,t] = min_r conditional(q,t,r) against the final state of
//             the others (+inf for a non-candidate), profile_rotamer[q,t] the smallest r attaining it (-1).
//   Outputs   aa_out (designed types; others as given); pos_out, mask_out as pf_pack_sidechains_fwd; designed_out; status; rotamer
//             (-1), chi (the chosen row; 0), n_candidates (0); energy_self_best = E_self of the start; energy_residue = E_self + half of
//             (P + F) at the end; energy_trace [B,sweeps+1] float64 ([0]: the start; sweeps not run repeat the last); sweeps_run;
//             changed, changed_types [B,sweeps] (residues whose (t, r), whose t changed in the sweep); profile, profile_rotamer;
//             choice_trace [B,sweeps,N,2] optional (type, rotamer at each visit; the caller fills it with -1 first).
//
// Arithmetic and summation order (fp32, -ffp-contract=off; pack_dev.h builds and evaluates, nothing there is reassociated):
//   E_self    mutscan.hip's order: a row atom's five term sums run over the column tiles ascending and the atoms of a tile ascending
//             (residue, slot), then its own residue's slots ascending; row energy e = (((w0 t0 + w1 t1) + w2 t2) + w3 t3) + w4 t4;
//             E_self = (((e_0 + e_1) + ... + e_8) + rot_energy) + ref_energy.  A designed residue's atoms are parked outside every
//             cutoff in the environment, and adding nothing is exact: with one designed residue and no ref_energy, E_self (and so
//             profile) has the bits of pf_mutation_scan_fwd's E.
//   P         a row atom's five sums over the other designed residues in ascending position, their 15 slots ascending; e as above;
//             P = (e_0 + e_1) + ... + e_8 (a slot the type lacks adds 0).
//   F         per partner residue, its existing rotamer atoms ascending, each with five sums over m's slots 0, 1, 2, 3, 4, 14: f =
//             ((0 + e_0) + e_1) + ...; then the 64 designed slots (absent and culled ones: 0) are added by a butterfly, v_i + v_(i ^ k),
//             k = 32, 16, .., 1, which gives every lane the same bits.
//   conditional = (E_self + P) + F.  energy_residue = E_self + 0.5 (P + F).
//   total     float64: designed residue m (thread m) adds E_self, then for m' ascending (m' != m) and its own rotamer atoms ascending
//             the row energy (fp32, five sums over the slots of m' ascending: the frame slots, and the rotamer slots when m' > m);
//             then a tree over the threads.
// Only pairs inside the cutoff are added, so culling does not show.  No atomics, one writer per output, nothing read back by the host:
// bit-identical from run to run and independent of the rest of the batch.
//   prep_kernel    a workgroup per sample: which residues are designed, their ascending list (<= 64; a residue's place is the count of
//                  designed residues in front of it, counted by its own thread), status; per residue the 15 environment atoms as
//                  float4 (a designed residue's all parked at x = -1e18), type bytes, bounds, slot.
//   self_kernel    the hot path.  Grid (20 types, max_res designed slots, B), 256 threads, as mutscan.hip's scan_kernel: rotamers
//                  built in registers and kept in LDS (18 KiB), rows compacted to the atoms the type has, environment tiles of 16
//                  residues double-buffered through LDS with broadcast reads.  E_self[m,t,r] goes to the workspace, 4 bytes an entry:
//                  no rotamer atom reaches global memory.  Also the extent of (m, t): the largest distance of any of its atoms from CA.
//   search_kernel  one workgroup per sample.  The current atoms of its <= 64 designed residues stay in LDS (15 KiB + type bytes); at a
//                  visit every candidate type's rotamers are rebuilt in registers into LDS (18 KiB) and scored against them; pairs of
//                  designed residues are culled by CA distance against E + E' + cutoff, E the extent over all candidates.  Start,
//                  sweeps, argmins, stop test, traces, totals, profile and the output structure are all done here.  LDS: 45 KiB.
//   Workspace      B (16 + 276 N + max_res (4 + 80 + 80 max_rot)) bytes: per residue 15 float4, a bound, 16 type bytes and a slot;
//                  per designed slot its residue, 20 extents and 20 max_rot E_self.  Nothing per N x type x rotamer x atom.
#include "pack_dev.h"

namespace {

using namespace pack_dev;

constexpr int NTYPES = PF_SEQ_DESIGN_TYPES, MAXD = PF_SEQ_DESIGN_MAX_RES;
constexpr long long BYTES_SAMPLE = 16, BYTES_RES = SL * 16 + 16 + 16 + 4, BYTES_SLOT = 4 + NTYPES * 4, BYTES_SLOT_ROT = NTYPES * 4;

struct Work {
    float4* env;                    // [B,N,15]
    float4* ebound;                 // [B,N] centre, extent of the residue's environment atoms (-1: none)
    unsigned char* envflg;          // [B,N,16]
    float* eself;                   // [B,max_res,20,R]
    float* ext;                     // [B,max_res,20] the largest distance of an atom of (slot, type) from CA
    int* dlist;                     // [B,max_res] the designed residues, ascending
    int* slot_of;                   // [B,N] the residue's place in dlist, -1: not designed
    int* ndes;                      // [B,4] the number of designed residues (0 when there are too many)
};

__host__ __device__ inline Work carve(void* work, size_t B, size_t N, size_t R, size_t MR) {
    Work w;
    char* p = static_cast<char*>(work);
    w.env = reinterpret_cast<float4*>(p);                   p += B * N * SL * sizeof(float4);
    w.ebound = reinterpret_cast<float4*>(p);                p += B * N * sizeof(float4);
    w.envflg = reinterpret_cast<unsigned char*>(p);         p += B * N * 16;
    w.eself = reinterpret_cast<float*>(p);                  p += B * MR * NTYPES * R * sizeof(float);
    w.ext = reinterpret_cast<float*>(p);                    p += B * MR * NTYPES * sizeof(float);
    w.dlist = reinterpret_cast<int*>(p);                    p += B * MR * sizeof(int);
    w.slot_of = reinterpret_cast<int*>(p);                  p += B * N * sizeof(int);
    w.ndes = reinterpret_cast<int*>(p);
    return w;
}

__device__ __forceinline__ bool is_designed(const pf_sequence_design_args& a, size_t i) {
    const long long aa = a.aa[i];
    const unsigned char* m = a.atom_mask + i * a.n_atoms;
    return a.designed[i] != 0 && aa >= 0 && aa <= 19 && m[0] != 0 && m[1] != 0 && m[2] != 0;
}

// the candidate types of the designed residue i as bits 0..19
__device__ __forceinline__ unsigned cand_bits(const pf_sequence_design_args& a, size_t i) {
    unsigned bits = 0;
    if (!a.candidates) {
        bits = (1u << NTYPES) - 1u;
    } else {
        for (int t = 0; t < NTYPES; ++t)
            if (a.candidates[i * NTYPES + t] != 0) bits |= 1u << t;
    }
    return bits ? bits : 1u << (int)a.aa[i];
}

__global__ __launch_bounds__(NT) void prep_kernel(pf_sequence_design_args a, Work w) {
    __shared__ int des[MAXN];
    const int N = a.N, A = a.n_atoms, MR = a.max_res, tid = threadIdx.x;
    const size_t b = blockIdx.x, row0 = b * N;
    for (int q = tid; q < N; q += NT) des[q] = is_designed(a, row0 + q) ? 1 : 0;
    __syncthreads();
    int total = 0;                                          // every thread counts for itself
    for (int q = 0; q < N; ++q) total += des[q];
    const bool over = total > MR, any = !over && total > 0;
    if (tid == 0) {
        w.ndes[b * 4] = over ? 0 : total;
        a.status[b] = over ? 1 : 0;
    }
    const float none[3] = {0.f, 0.f, 0.f};
    for (int q = tid; q < N; q += NT) {
        const size_t i = row0 + q;
        const bool d = any && des[q] != 0;
        int before = 0;                                     // the designed residues in front of q: its place in the ascending list
        for (int k = 0; k < q; ++k) before += des[k];
        if (d) w.dlist[b * MR + before] = q;
        const int t = type_row(a.aa[i]);
        float4 e[SL];
        unsigned char flg[SL];
        env_atoms(a, t, a.atom_mask + i * A, a.pos + i * A * 3, A, false, none, e, flg);
        for (int s = 0; s < SL; ++s) {
            if (d) e[s] = make_float4(-FAR, 0.f, 0.f, 0.f);     // a designed residue is not environment
            w.env[i * SL + s] = e[s];
            w.envflg[i * 16 + s] = flg[s];
        }
        w.envflg[i * 16 + 15] = 0;
        w.ebound[i] = env_bound(e);
        w.slot_of[i] = d ? before : -1;
        a.designed_out[i] = d;
        a.n_candidates[i] = d ? __popc(cand_bits(a, i)) : 0;
    }
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
__device__ __forceinline__ Fetched fetch_tile(const pf_sequence_design_args& a, const Work& w, size_t b, int ct, int tid) {
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

struct SelfLds {
    Tile tile[2];
    float4 rot[MAXR * RA];          // every rotamer of the type, built here
    float4 own[SL];                 // the residue's fixed atoms as type t has them
    float erow[MAXR * RA];          // row energies
    int list[MAX_TILES];
    int n_list;
    int live[RA], na;               // the rotamer atoms the type has, ascending
    float wave_max[NT / 64];
};

// The twin of mutscan.hip's scan_kernel (with its Tile, Fetched, fetch_tile, commit_tile): the same rows, tiles, sums and order,
// without the group sums, plus the ref_energy add.  profile's bit-equality with pf_mutation_scan_fwd rests on the two staying in step
// (tests/test_gpu_seqdesign.py: test_bitwise_against_mutation_scan): a change to the one belongs in the other.
__global__ __launch_bounds__(NT) void self_kernel(pf_sequence_design_args a, Work w) {
    __shared__ SelfLds L;
    const int N = a.N, R = a.max_rot, A = a.n_atoms, MR = a.max_res, tid = threadIdx.x, t = blockIdx.x, m = blockIdx.y;
    const size_t b = blockIdx.z;
    if (m >= w.ndes[b * 4]) return;                         // (the whole workgroup)
    const int q = w.dlist[b * MR + m];
    const size_t i = b * N + q, o = (b * MR + m) * NTYPES + t;
    if (!((cand_bits(a, i) >> t) & 1u)) return;
    const int cnt = rot_count(a, t), n_tiles = (N + TR - 1) / TR;
    const float cutoff = a.cutoff, cut2 = cutoff * cutoff;
    const unsigned char* mk = a.atom_mask + i * A;
    const float* p = a.pos + i * A * 3;

    Backbone F;
    backbone_frame(a, t, p, true, F);
    if (tid == 0) {                                         // the own residue's fixed atoms, as type t
        float4 e[SL];
        unsigned char flg[SL];
        env_atoms(a, t, mk, p, A, true, F.cb, e, flg);
        for (int s = 0; s < SL; ++s) L.own[s] = e[s];
    }
    float ext = 0.f;
    if (tid < cnt) {
        float4* dst = L.rot + tid * RA;
        for (int j = 0; j < RA; ++j) dst[j] = make_float4(FAR, 0.f, 0.f, 0.f);
        ext = build_rotamer(a, t, a.rot_chi + ((size_t)t * R + tid) * 4, F, [dst](int j, const float4& v) { dst[j] = v; });
    }
    for (int k = tid; k < cnt * RA; k += NT) L.erow[k] = 0.f;
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
            float x = C.w;                                  // the extent of (m, t): rotamer atoms and fixed atoms
            for (int s = 0; s < SL; ++s)
                if (L.own[s].w > 0.f) x = fmaxf(x, dist3(L.own[s], C));
            w.ext[o] = x;
        }
    }
    __syncthreads();
    const int n = L.n_list, na = L.na, rows = cnt * na;
    const long long my_idx = a.residue_index[i];

    for (int row0 = 0; row0 < rows; row0 += NT) {
        const bool has = row0 + tid < rows;
        const int r = has ? (row0 + tid) / na : 0, j = has ? L.live[(row0 + tid) % na] : 0;
        const float4 P = has ? L.rot[r * RA + j] : make_float4(FAR, 0.f, 0.f, 0.f);
        const unsigned char fp = a.types[t * SL + S0 + j];
        const bool my_sg = t == a.cys && j == 0;
        const int pro_excl = t == a.pro ? (j == 1 ? 0xE : j == 0 ? 0x4 : 0) : 0;   // CD: CA, C, O; CG: C of the previous residue
        float ts[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (n > 0) {
            commit_tile(L.tile[0], fetch_tile(a, w, b, L.list[0], tid), tid);
            __syncthreads();
        }
        for (int k = 0; k < n; ++k) {                       // the environment: the residues that are not designed
            Fetched next;
            const bool more = k + 1 < n;
            if (more) next = fetch_tile(a, w, b, L.list[k + 1], tid);
            const Tile& T = L.tile[k & 1];
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
            if (more) commit_tile(L.tile[(k + 1) & 1], next, tid);
            __syncthreads();
        }
        if (has) {
            const int own = a.own_mask[t * SL + S0 + j];    // the own residue, slots ascending
            for (int s = 0; s < SL; ++s) {
                if (!((own >> s) & 1)) continue;
                const float4 v = (s < S0 || s == 14) ? L.own[s] : L.rot[r * RA + (s - S0)];
                if (v.w > 0.f) pair_add(P, fp, v, a.types[t * SL + s], cut2, ts);
            }
            L.erow[r * RA + j] = weighted(a, ts);
        }
    }
    __syncthreads();
    if (tid < cnt) {
        float e = L.erow[tid * RA];
        for (int k = 1; k < RA; ++k) e += L.erow[tid * RA + k];
        e = e + a.rot_energy[(size_t)t * R + tid];
        if (a.ref_energy) e = e + a.ref_energy[t];
        w.eself[o * R + tid] = e;
    }
}

struct SearchLds {
    float4 cur[MAXD * SL];          // the current atoms of the designed residues (absent: x = -1e18, radius 0)
    unsigned char cflg[MAXD * 16];  // their type bytes
    float4 bound[MAXD];             // CA, extent over all candidates
    float4 rot[MAXR * RA];          // a visit: every rotamer of the candidate type
    float erow[MAXR * RA];
    float4 own[SL];                 //          the visited residue's frame atoms under the candidate type
    unsigned char oflg[16];
    int q[MAXD], idx[MAXD], typ[MAXD], rotm[MAXD];
    unsigned cand[MAXD];
    int live[RA], na;
    float fval;
    float best_v[NT / 64];
    int best_i[NT / 64];
    double red[NT];
    int n_changed, n_changed_t;
};

__device__ __forceinline__ bool near_pair(const SearchLds& L, int p, int p2, float cutoff) {
    const float4 u = L.bound[p], v = L.bound[p2];
    return L.idx[p] != L.idx[p2] && dist3(u, v) <= ((u.w + v.w) + cutoff) * CULL_SLACK + CULL_ABS;
}

// the PRO rotamer atom j (CG: 0, CD: 1) does not see these slots of the previous residue
__device__ __forceinline__ int pro_mask(int j) { return j == 1 ? 0xE : j == 0 ? 0x4 : 0; }

// one thread: the current atoms and type bytes of designed residue p become those of (t, r)
__device__ void place(const pf_sequence_design_args& a, SearchLds& L, size_t i, int p, int t, int r) {
    const int A = a.n_atoms;
    const float* ps = a.pos + i * A * 3;
    Backbone F;
    backbone_frame(a, t, ps, true, F);
    float4 e[SL];
    unsigned char flg[SL];
    env_atoms(a, t, a.atom_mask + i * A, ps, A, true, F.cb, e, flg);
    float4* dst = L.cur + p * SL;
    for (int s = 0; s < SL; ++s) {
        dst[s] = e[s];
        L.cflg[p * 16 + s] = flg[s];
    }
    L.cflg[p * 16 + 15] = 0;
    build_rotamer(a, t, a.rot_chi + ((size_t)t * a.max_rot + r) * 4, F, [dst](int j, const float4& v) { dst[S0 + j] = v; });
}

// All threads: the conditional energies of every candidate (t, r) of designed residue p against the current state of the others.
// -> the argmin (bt, br) under (value, t, r), the same in every thread.  PROFILE: also writes profile, profile_rotamer and
// energy_residue of p's row.  Ends with the LDS it used free for the next call (a barrier).
template <bool PROFILE>
__device__ void visit(const pf_sequence_design_args& a, const Work& w, SearchLds& L, size_t b, int p, int n, int& bt, int& br) {
    const int N = a.N, R = a.max_rot, A = a.n_atoms, tid = threadIdx.x;
    const float cutoff = a.cutoff, cut2 = cutoff * cutoff;
    const size_t i = b * N + L.q[p], slot = b * a.max_res + p;
    const unsigned cand = L.cand[p];
    const int my_idx = L.idx[p];
    const unsigned char* mk = a.atom_mask + i * A;
    const float* ps = a.pos + i * A * 3;
    float run_v = INFINITY;
    bt = -1;
    br = 0;
    for (int t = 0; t < NTYPES; ++t) {
        const size_t o = i * NTYPES + t;
        if (!((cand >> t) & 1u)) {
            if (PROFILE && tid == 0) {
                a.profile[o] = INFINITY;
                a.profile_rotamer[o] = -1;
            }
            continue;
        }
        const int cnt = rot_count(a, t);
        Backbone F;
        backbone_frame(a, t, ps, true, F);
        if (tid == 0) {
            float4 e[SL];
            unsigned char flg[SL];
            env_atoms(a, t, mk, ps, A, true, F.cb, e, flg);
            for (int s = 0; s < SL; ++s) {
                L.own[s] = e[s];
                L.oflg[s] = flg[s];
            }
        }
        if (tid < cnt) {
            float4* dst = L.rot + tid * RA;
            for (int j = 0; j < RA; ++j) dst[j] = make_float4(FAR, 0.f, 0.f, 0.f);
            build_rotamer(a, t, a.rot_chi + ((size_t)t * R + tid) * 4, F, [dst](int j, const float4& v) { dst[j] = v; });
        }
        for (int k = tid; k < cnt * RA; k += NT) L.erow[k] = 0.f;
        __syncthreads();
        if (tid == 0) {
            int na = 0;
            for (int j = 0; j < RA; ++j)
                if (L.rot[j].w > 0.f) L.live[na++] = j;
            L.na = na;
        }
        __syncthreads();

        if (tid < 64) {                                     // F: wave 0, a designed slot per lane
            float f = 0.f;
            const int p2 = tid;
            if (p2 < n && p2 != p && near_pair(L, p, p2, cutoff)) {
                const bool bonded = L.typ[p2] == a.pro && my_idx + 1 == L.idx[p2];
                for (int j = 0; j < RA; ++j) {
                    const float4 P = L.cur[p2 * SL + S0 + j];
                    if (!(P.w > 0.f)) continue;
                    const unsigned char fp = L.cflg[p2 * 16 + S0 + j];
                    const int excl = bonded ? pro_mask(j) : 0;
                    float ts[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
                    for (int s = 0; s < SL; ++s) {
                        if (s >= S0 && s != 14) continue;
                        const float4 v = L.own[s];
                        if (v.w > 0.f && !((excl >> s) & 1)) pair_add(P, fp, v, L.oflg[s], cut2, ts);
                    }
                    f += weighted(a, ts);
                }
            }
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) f = f + __shfl_xor(f, k);
            if (tid == 0) L.fval = f;
        }

        const int na = L.na, rows = cnt * na;
        for (int row0 = 0; row0 < rows; row0 += NT) {       // P
            const bool has = row0 + tid < rows;
            const int r = has ? (row0 + tid) / na : 0, j = has ? L.live[(row0 + tid) % na] : 0;
            const float4 P = has ? L.rot[r * RA + j] : make_float4(FAR, 0.f, 0.f, 0.f);
            const unsigned char fp = a.types[t * SL + S0 + j];
            const bool my_sg = t == a.cys && j == 0;
            const int pro_excl = t == a.pro ? pro_mask(j) : 0;
            float ts[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            for (int p2 = 0; p2 < n; ++p2) {
                if (p2 == p || !near_pair(L, p, p2, cutoff)) continue;
                const int excl = L.idx[p2] + 1 == my_idx ? pro_excl : 0;
#pragma unroll 5
                for (int s = 0; s < SL; ++s) {
                    const float4 v = L.cur[p2 * SL + s];
                    const unsigned char f = L.cflg[p2 * 16 + s];
                    if (!((excl >> s) & 1) && !(my_sg && (f & IS_SG))) pair_add(P, fp, v, f, cut2, ts);
                }
            }
            if (has) L.erow[r * RA + j] = weighted(a, ts);
        }
        __syncthreads();

        float es = 0.f, e = 0.f, c = 0.f, v = INFINITY;
        int vi = 0x7fffffff;
        if (tid < cnt) {                                    // cnt <= 128: waves 0 and 1
            e = L.erow[tid * RA];
            for (int k = 1; k < RA; ++k) e += L.erow[tid * RA + k];
            es = w.eself[(slot * NTYPES + t) * R + tid];
            c = (es + e) + L.fval;
            v = no_nan(c);
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
        const bool second = better(L.best_v[1], L.best_i[1], L.best_v[0], L.best_i[0]);
        const float tv = second ? L.best_v[1] : L.best_v[0];
        const int tr = second ? L.best_i[1] : L.best_i[0];
        if (bt < 0 || tv < run_v) {                         // types ascending: a tie stays with the smaller t
            run_v = tv;
            bt = t;
            br = tr;
        }
        if (PROFILE) {
            if (tid == tr) {                                // one writer: the thread that holds the chosen rotamer's energies
                a.profile[o] = c;
                a.profile_rotamer[o] = tr;
            }
            if (t == L.typ[p] && tid == L.rotm[p]) a.energy_residue[i] = es + 0.5f * (e + L.fval);
        }
    }
    __syncthreads();
}

__device__ double total_energy(const pf_sequence_design_args& a, const Work& w, SearchLds& L, size_t b, int n, int tid) {
    const float cutoff = a.cutoff, cut2 = cutoff * cutoff;
    double acc = 0.0;
    if (tid < n) {
        const int p = tid, my_idx = L.idx[p];
        acc = (double)w.eself[((b * a.max_res + p) * NTYPES + L.typ[p]) * a.max_rot + L.rotm[p]];
        const bool pro = L.typ[p] == a.pro;
        for (int p2 = 0; p2 < n; ++p2) {
            if (p2 == p || !near_pair(L, p, p2, cutoff)) continue;
            const bool bonded = pro && L.idx[p2] + 1 == my_idx;
            for (int j = 0; j < RA; ++j) {
                const float4 P = L.cur[p * SL + S0 + j];
                if (!(P.w > 0.f)) continue;
                const unsigned char fp = L.cflg[p * 16 + S0 + j];
                const bool my_sg = (fp & IS_SG) != 0;
                const int excl = bonded ? pro_mask(j) : 0;
                float ts[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
                for (int s = 0; s < SL; ++s) {
                    if (s >= S0 && s != 14 && p2 < p) continue;     // rotamer against rotamer: each pair once
                    const unsigned char f = L.cflg[p2 * 16 + s];
                    if (!((excl >> s) & 1) && !(my_sg && (f & IS_SG))) pair_add(P, fp, L.cur[p2 * SL + s], f, cut2, ts);
                }
                acc += (double)weighted(a, ts);
            }
        }
    }
    return block_sum<NT>(acc, L.red, tid);
}

__global__ __launch_bounds__(NT) void search_kernel(pf_sequence_design_args a, Work w) {
    __shared__ SearchLds L;
    const int N = a.N, R = a.max_rot, A = a.n_atoms, MR = a.max_res, tid = threadIdx.x, S = a.sweeps;
    const size_t b = blockIdx.x, row0 = b * N;
    const int n = w.ndes[b * 4];

    for (int p = tid; p < n; p += NT) {
        const int q = w.dlist[b * MR + p];
        const size_t i = row0 + q;
        const unsigned cand = cand_bits(a, i);
        L.q[p] = q;
        L.idx[p] = a.residue_index[i];
        L.cand[p] = cand;
        float x = 0.f;
        for (int t = 0; t < NTYPES; ++t)
            if ((cand >> t) & 1u) x = fmaxf(x, w.ext[(b * MR + p) * NTYPES + t]);
        const float* ca = a.pos + (i * A + 1) * 3;
        L.bound[p] = make_float4(ca[0], ca[1], ca[2], x);
    }
    __syncthreads();
    for (int p = tid >> 6; p < n; p += NT / 64) {           // the start: a wave per residue, argmin of E_self under (value, t, r)
        const unsigned cand = L.cand[p];
        const float* es = w.eself + (b * MR + p) * NTYPES * (size_t)R;
        float v = INFINITY;
        int vi = 0x7fffffff;
        for (int k = tid & 63; k < NTYPES * R; k += 64) {
            const int t = k / R, r = k % R;
            if (!((cand >> t) & 1u) || r >= rot_count(a, t)) continue;
            const float x = no_nan(es[k]);
            if (better(x, k, v, vi)) {
                v = x;
                vi = k;
            }
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
        if ((tid & 63) == 0) {                              // (a candidate set is never empty, so vi is an entry)
            L.typ[p] = vi / R;
            L.rotm[p] = vi % R;
            a.energy_self_best[row0 + L.q[p]] = es[vi];
        }
    }
    __syncthreads();
    if (tid < n) place(a, L, row0 + L.q[tid], tid, L.typ[tid], L.rotm[tid]);
    __syncthreads();

    double* trace = a.energy_trace + b * (S + 1);
    double e_now = total_energy(a, w, L, b, n, tid);
    if (tid == 0) trace[0] = e_now;
    int run = 0;
    for (int sweep = 0; sweep < S; ++sweep) {
        if (tid == 0) L.n_changed = L.n_changed_t = 0;
        for (int p = 0; p < n; ++p) {
            int bt, br;
            visit<false>(a, w, L, b, p, n, bt, br);
            const bool moved_t = bt != L.typ[p], moved = moved_t || br != L.rotm[p];
            __syncthreads();                                // every thread has read typ[p] and rotm[p]
            if (tid == 0) {
                if (moved) {
                    place(a, L, row0 + L.q[p], p, bt, br);
                    L.typ[p] = bt;
                    L.rotm[p] = br;
                    L.n_changed += 1;
                    L.n_changed_t += moved_t;
                }
                if (a.choice_trace) {
                    int* c = a.choice_trace + (((size_t)b * S + sweep) * N + L.q[p]) * 2;
                    c[0] = bt;
                    c[1] = br;
                }
            }
            __syncthreads();
        }
        e_now = total_energy(a, w, L, b, n, tid);
        const int changed = L.n_changed;
        if (tid == 0) {
            trace[sweep + 1] = e_now;
            a.changed[b * S + sweep] = changed;
            a.changed_types[b * S + sweep] = L.n_changed_t;
        }
        run = sweep + 1;
        __syncthreads();                                    // the counts are reset at the top of the next sweep
        if (changed == 0) break;
    }
    if (tid == 0) {
        a.sweeps_run[b] = run;
        for (int s = run; s < S; ++s) {
            trace[s + 1] = e_now;
            a.changed[b * S + s] = 0;
            a.changed_types[b * S + s] = 0;
        }
    }

    for (int p = 0; p < n; ++p) {                           // the profile against the final state
        int bt, br;
        visit<true>(a, w, L, b, p, n, bt, br);
    }

    for (int q = tid; q < N; q += NT) {
        const size_t i = row0 + q;
        const int p = w.slot_of[i];
        const int t = p >= 0 ? L.typ[p] : type_row(a.aa[i]), r = p >= 0 ? L.rotm[p] : -1;
        a.aa_out[i] = p >= 0 ? (long long)t : a.aa[i];
        a.rotamer[i] = r;
        if (p < 0) {
            a.energy_self_best[i] = 0.f;
            a.energy_residue[i] = 0.f;
            for (int k = 0; k < NTYPES; ++k) {
                a.profile[i * NTYPES + k] = INFINITY;
                a.profile_rotamer[i * NTYPES + k] = -1;
            }
        }
        for (int k = 0; k < 4; ++k) a.chi[i * 4 + k] = p >= 0 ? a.rot_chi[((size_t)t * R + r) * 4 + k] : 0.f;
    }
    for (int k = tid; k < N * SL; k += NT) {
        const int q = k / SL, s = k % SL;
        const size_t i = row0 + q;
        const int p = w.slot_of[i];
        float x[3] = {0.f, 0.f, 0.f};
        unsigned char mk = 0;
        if (p < 0 || s < 4 || s == 14) {                    // the input's bits
            if (s < A) {
                const float* ps = a.pos + (i * A + s) * 3;
                x[0] = ps[0]; x[1] = ps[1]; x[2] = ps[2];
                mk = a.atom_mask[i * A + s];
            }
        } else {
            mk = a.tab_mask[L.typ[p] * SL + s];
            const float4 v = L.cur[p * SL + s];
            if (mk && v.w > 0.f) { x[0] = v.x; x[1] = v.y; x[2] = v.z; }
        }
        float* o = a.pos_out + (i * SL + s) * 3;
        o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
        a.mask_out[i * SL + s] = mk;
    }
}

__host__ inline bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" int pf_sequence_design_work_bytes(int B, int N, int max_rot, int max_res) {
    if (B < 0 || N < 0 || N > PF_PACK_MAX_N || max_rot < 1 || max_rot > PF_PACK_MAX_ROT || max_res < 1 || max_res > PF_SEQ_DESIGN_MAX_RES)
        return -1;
    const long long bytes = (long long)B * (BYTES_SAMPLE + BYTES_RES * N + (long long)max_res * (BYTES_SLOT + BYTES_SLOT_ROT * max_rot));
    return bytes > 0x7fffffffLL ? -1 : (int)bytes;
}

extern "C" int pf_sequence_design_fwd(const pf_sequence_design_args* a, pf_stream_t stream) {
    if (!a || !a->pos || !a->atom_mask || !a->aa || !a->residue_index || !a->designed || !a->radius || !a->types || !a->own_mask ||
        !a->tab_rot || !a->tab_trans || !a->tab_group || !a->tab_pos || !a->tab_mask || !a->rot_chi || !a->rot_count ||
        !a->rot_energy || !a->work || !a->aa_out || !a->pos_out || !a->mask_out || !a->designed_out || !a->status || !a->rotamer ||
        !a->chi || !a->n_candidates || !a->energy_self_best || !a->energy_residue || !a->energy_trace || !a->sweeps_run ||
        ((!a->changed || !a->changed_types) && a->sweeps > 0) || !a->profile || !a->profile_rotamer || a->B < 0 || a->N < 0 ||
        a->n_atoms < SL - 1 || a->max_rot < 1 || a->max_res < 1 || a->sweeps < 0 || !(a->cutoff > 0.f) || !(a->cutoff < 1e6f) ||
        !finite_f(a->w_gauss1) || !finite_f(a->w_gauss2) || !finite_f(a->w_repulsion) || !finite_f(a->w_hydrophobic) ||
        !finite_f(a->w_hbond))
        return PF_E_BADARG;
    if (a->N > PF_PACK_MAX_N || a->max_rot > PF_PACK_MAX_ROT || a->max_res > PF_SEQ_DESIGN_MAX_RES || a->B > 65535) return PF_E_TOOLARGE;
    if (pf_sequence_design_work_bytes(a->B, a->N, a->max_rot, a->max_res) < 0) return PF_E_TOOLARGE;
    if (a->B == 0 || a->N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const Work w = carve(a->work, (size_t)a->B, (size_t)a->N, (size_t)a->max_rot, (size_t)a->max_res);
    hipLaunchKernelGGL(prep_kernel, dim3((unsigned)a->B), dim3(NT), 0, st, *a, w);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(self_kernel, dim3(NTYPES, (unsigned)a->max_res, (unsigned)a->B), dim3(NT), 0, st, *a, w);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(search_kernel, dim3((unsigned)a->B), dim3(NT), 0, st, *a, w);
    PF_CHECK_LAUNCH();
    return 0;
}
