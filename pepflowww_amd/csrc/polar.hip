// pf_polar_fwd -- hydrogen bonds and salt bridges between the heavy atoms of different residues of a batch of structures, with the
// explicit list of which atom bonds which.  Heavy atoms only (the package has no hydrogens), by the published heavy-atom conventions:
// donor-acceptor distance and antecedent angles (Baker & Hubbard, Prog. Biophys. Mol. Biol. 44, 1984; McDonald & Thornton, J. Mol.
// Biol. 238, 1994) and the N-O distance of a salt bridge (Barlow & Thornton, J. Mol. Biol. 168, 1983).  Written from the publications;
// checked against the float64 restatement tests/polar_oracle.py and constructed cases.  It is NOT checked against HBPLUS, PLIP or
// Rosetta and is none of their outputs (no hydrogens placed, no tautomers, no water, no terminal charges).
//
// Conventions (tests/polar_oracle.py restates them in numpy float64):
//   Atoms     slots 0 .. min(n_atoms, 15) - 1 of pos [B,N,n_atoms,3] in the package's heavy-atom order (0 N, 2 C, 3 O, 14 OXT),
//             n_atoms >= 14.  An atom takes part where atom_mask is set and the residue type has the slot: antecedents [21,15,2] has a
//             first entry >= 0 there, every heavy atom being bonded to another of its residue (a type outside 0..19 reads row 20:
//             N, CA, C, O).
//   Typing    types [21,15]: bit 1 donor, bit 2 acceptor (geometry.interface_type_table; bit 0 is ignored); charge [21,15]: 1 cation N,
//             2 anion O (geometry.charge_table).
//   Antecedents  of atom X: the participating atoms among the (up to two) bonded slots of antecedents[type][slot], and for the
//             backbone N (slot 0) also C (slot 2) of the previous row when residue_index[i-1] + 1 == residue_index[i] and that C
//             takes part.  An atom without a participating antecedent passes its angle test vacuously.
//   H-bond    atoms p, q of different residues; tried with p as donor D and q as acceptor A and the other way round where the type
//             bits allow, either passing counts once:  |D - A|^2 <= d_max^2;  for every antecedent X of A the angle X-A...D >=
//             acc_angle_min, as  (X - A).(D - A) <= cos_acc * (|X - A| * |D - A|);  for every antecedent Y of D the angle Y-D...A >=
//             don_angle_min likewise with cos_don.  No acos.  Excluded: the backbone N of residue i with O or OXT (slots 3, 14) of
//             residue i - 1 when the two are chain-consecutive (a 1-3 pair).
//   Salt      a cation N and an anion O of different residues with |p - q|^2 <= salt_max^2, independent of the hydrogen-bond test.
//   Outputs   per row atom: hbonds_atom, salt_atom [B,N,15] int32 = its partners; with group the _cross twins = the partners whose
//             residue has another group byte; hbond_partner, salt_partner [B,N,15,4] = residue * 15 + slot of the partners in ascending
//             order, the 4 lowest, padded with -1 (the count stays exact).  Per row residue: the sums over its slots.  Each pair
//             shows in both of its rows.
//   query     [B,N]: only atoms of query residues are rows; every participating atom is still a partner.  A participating atom that
//             is not a row has the counts -1 and empty lists, as in pf_interface_energy_fwd; it adds nothing to its residue's sums.
//
// Two launches, no atomics, nothing pair-sized: every output has one writer and the lists are filled in scan order (column tiles
// ascending, the atoms of a tile ascending), which is ascending in residue * 15 + slot, so nothing is sorted.  A decision is computed
// from (D, A) in that order whichever of the two is the row, with the same operations: the two rows of a pair agree bit for bit.
//   bounds_kernel  a thread per residue: work [B,N,4] = (centre, extent): the coordinates of its CA (or of its first participating atom)
//                  and the largest distance of a participating donor, acceptor or charged atom from it (-1: no such atom).
//   polar_kernel   grid (row tiles of 16 residues, B), 256 threads; thread t < 240 owns row atom (t / 15, t % 15), keeps the
//                  coordinates of its own antecedents in registers and walks every atom of every kept column tile.  Column tiles are
//                  staged in LDS, double-buffered: float4 (x, y, z, -) per atom, a flag byte, the two antecedent slots already
//                  resolved to participating atoms (their coordinates are the same tile's: an antecedent is of the same residue), and
//                  per residue the previous row's C (w = 1: it is an antecedent of N), the chain-consecutive flag and the group byte.
//                  All lanes of a wave read the SAME column atom in a step: a broadcast.  An atom that does not take part is parked
//                  at x = +1e18 (row) / -1e18 (column); a row atom without any polar bit is parked too.  The angle tests run only
//                  for the few pairs inside the distance.  Wave 0 builds the list of column tiles to visit, a tile per lane: those
//                  holding a residue within (E + e_q + max(d_max, salt_max)) of the row tile's centre (a superset).  The slots of a
//                  residue are summed through LDS by one thread per residue.
#include "common.h"
#include "../../include/pepflow_hip.h"
#include "eval_dev.h"

namespace {

constexpr int TR = 16, SL = 15, TA = TR * SL;               // residues per tile, slots per residue, atoms per tile
constexpr int NT = 256;
constexpr int MAX_TILES = PF_POLAR_MAX_N / TR;
constexpr int K = PF_POLAR_MAX_PARTNERS;
constexpr int SLOT_N = 0, SLOT_C = 2, SLOT_O = 3, SLOT_OXT = 14;
constexpr float FAR = 1e18f;
constexpr float CULL_SLACK = 1.0001f;
constexpr unsigned char DONOR = 2, ACCEPTOR = 4, CATION = 8, ANION = 16;        // the tile's flag byte: type bits 1, 2; charge << 3

struct Tile {
    float4 a[TA];                   // x, y, z
    float4 prev_c[TR];              // C of the previous row; w = 1 where it is an antecedent of the residue's N
    unsigned char flg[TA];
    signed char ant[TA][2];         // antecedent slots that take part, -1: none
    unsigned char grp[TR];
    unsigned char consec[TR];       // residue_index[q - 1] + 1 == residue_index[q]
};

struct Fetched {
    float4 a, prev_c;
    unsigned char flg, exists, grp, consec;
    signed char ant0, ant1;
};

struct Ants {                       // the antecedents of one atom
    float4 x[3];
    bool has[3];
};

__device__ __forceinline__ float dist3(const float4& p, const float4& q) {
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

__device__ __forceinline__ float4 load_atom(const float* p) { return make_float4(p[0], p[1], p[2], 0.f); }

// the angle X-P...Q is at least the one whose cosine is c
__device__ __forceinline__ bool angle_ok(const float4& X, const float4& P, const float4& Q, float c) {
    const float ux = X.x - P.x, uy = X.y - P.y, uz = X.z - P.z;
    const float vx = Q.x - P.x, vy = Q.y - P.y, vz = Q.z - P.z;
    const float dot = (ux * vx + uy * vy) + uz * vz;
    const float uu = (ux * ux + uy * uy) + uz * uz, vv = (vx * vx + vy * vy) + vz * vz;
    return dot <= c * (sqrtf(uu) * sqrtf(vv));
}

// donor D with antecedents dy, acceptor A with antecedents ax; the distance has been tested
__device__ __forceinline__ bool angles_ok(const float4& D, const Ants& dy, const float4& A, const Ants& ax, float cos_acc, float cos_don) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (ax.has[k]) ok = ok && angle_ok(ax.x[k], A, D, cos_acc);
        if (dy.has[k]) ok = ok && angle_ok(dy.x[k], D, A, cos_don);
    }
    return ok;
}

__device__ __forceinline__ bool takes_part(const pf_polar_args& a, size_t r, int tr, int s) {
    return a.atom_mask[r * a.n_atoms + s] != 0 && a.antecedents[(tr * SL + s) * 2] >= 0;
}

__global__ __launch_bounds__(256) void bounds_kernel(pf_polar_args a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.B * a.N) return;
    const int A = a.n_atoms, S = A < SL ? A : SL;
    const float* p = a.pos + i * A * 3;
    const int tr = type_row(a.aa[i]);
    int c = -1;                                             // slot 1 (CA) if it takes part, else the first slot that does
    if (takes_part(a, i, tr, 1)) c = 1;
    for (int s = 0; s < S && c < 0; ++s)
        if (takes_part(a, i, tr, s)) c = s;
    float4 w = make_float4(0.f, 0.f, 0.f, -1.f);
    if (c >= 0) {
        w = make_float4(p[3 * c], p[3 * c + 1], p[3 * c + 2], -1.f);
        const float4 centre = w;
        for (int s = 0; s < S; ++s)
            if (takes_part(a, i, tr, s) && ((a.types[tr * SL + s] & (DONOR | ACCEPTOR)) != 0 || a.charge[tr * SL + s] != 0))
                w.w = fmaxf(w.w, dist3(load_atom(p + 3 * s), centre));
    }
    reinterpret_cast<float4*>(a.work)[i] = w;
}

// thread t < 240: atom t of tile ct of structure b (one that does not take part: x = far); thread t < 16: residue t of it.  Every
// address is formed only for q < N, s < n_atoms.
__device__ __forceinline__ Fetched fetch_tile(const pf_polar_args& a, size_t b, int ct, int tid, float far) {
    Fetched f;
    f.a = make_float4(far, 0.f, 0.f, 0.f);
    f.prev_c = make_float4(0.f, 0.f, 0.f, 0.f);
    f.flg = f.exists = f.grp = f.consec = 0;
    f.ant0 = f.ant1 = -1;
    const int N = a.N, A = a.n_atoms;
    if (tid < TA) {
        const int q = ct * TR + tid / SL, s = tid % SL;
        if (q < N && s < A) {
            const size_t r = b * N + q;
            const int tr = type_row(a.aa[r]);
            if (takes_part(a, r, tr, s)) {
                f.a = load_atom(a.pos + (r * A + s) * 3);
                f.flg = (unsigned char)((a.types[tr * SL + s] & (DONOR | ACCEPTOR)) | (a.charge[tr * SL + s] << 3));
                f.exists = 1;
                const signed char a0 = a.antecedents[(tr * SL + s) * 2], a1 = a.antecedents[(tr * SL + s) * 2 + 1];
                if (a0 >= 0 && a0 < A && a0 < SL && a.atom_mask[r * A + a0] != 0) f.ant0 = a0;
                if (a1 >= 0 && a1 < A && a1 < SL && a.atom_mask[r * A + a1] != 0) f.ant1 = a1;
            }
        }
    }
    if (tid < TR) {
        const int q = ct * TR + tid;
        if (q < N) {
            if (a.group) f.grp = a.group[b * N + q];
            if (q > 0 && a.residue_index[b * N + q - 1] + 1 == a.residue_index[b * N + q]) {
                f.consec = 1;
                const size_t r = b * N + q - 1;
                if (takes_part(a, r, type_row(a.aa[r]), SLOT_C)) {
                    f.prev_c = load_atom(a.pos + (r * A + SLOT_C) * 3);
                    f.prev_c.w = 1.f;
                }
            }
        }
    }
    return f;
}

__device__ __forceinline__ void commit_tile(Tile& t, const Fetched& f, int tid) {
    if (tid < TA) {
        t.a[tid] = f.a;
        t.flg[tid] = f.flg;
        t.ant[tid][0] = f.ant0;
        t.ant[tid][1] = f.ant1;
    }
    if (tid < TR) {
        t.prev_c[tid] = f.prev_c;
        t.grp[tid] = f.grp;
        t.consec[tid] = f.consec;
    }
}

__global__ __launch_bounds__(NT) void polar_kernel(pf_polar_args a) {
    __shared__ Tile tile[2];
    __shared__ unsigned char row_grp[TR];
    __shared__ int list[MAX_TILES];
    __shared__ int n_list;
    __shared__ int red[4][TA];
    const int N = a.N, A = a.n_atoms, tid = threadIdx.x;
    const size_t b = blockIdx.y;
    const int rt = blockIdx.x, n_tiles = (N + TR - 1) / TR;
    const int r0 = rt * TR, r1 = r0 + TR < N ? r0 + TR : N;
    const float dmax2 = a.d_max * a.d_max, salt2 = a.salt_max * a.salt_max, cut2 = fmaxf(dmax2, salt2);
    const float reach = fmaxf(a.d_max, a.salt_max);
    const float cos_acc = a.cos_acc, cos_don = a.cos_don;
    const unsigned char* query = a.query ? a.query + b * N : nullptr;
    const bool grouped = a.group != nullptr;
    const float4* work = reinterpret_cast<const float4*>(a.work) + b * N;

    // the thread's row atom: parked unless it takes part, has a polar bit and its residue is a row
    Fetched me = fetch_tile(a, b, rt, tid, FAR);
    const int rr = tid < TA ? tid / SL : 0, my_s = tid < TA ? tid % SL : 0, my_r = r0 + rr;
    const bool is_row = me.exists && (!query || query[my_r] != 0);
    if (!is_row || me.flg == 0) me.a = make_float4(FAR, 0.f, 0.f, 0.f);
    if (tid < TR) row_grp[tid] = me.grp;

    // its antecedents: the bonded atoms of its residue that take part, and for N the previous row's C
    Ants mine;
    for (int k = 0; k < 3; ++k) {
        mine.x[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        mine.has[k] = false;
    }
    bool my_consec = false;
    if (is_row && me.flg != 0) {
        const size_t r = b * N + my_r;
        if (me.ant0 >= 0) {
            mine.x[0] = load_atom(a.pos + (r * A + me.ant0) * 3);
            mine.has[0] = true;
        }
        if (me.ant1 >= 0) {
            mine.x[1] = load_atom(a.pos + (r * A + me.ant1) * 3);
            mine.has[1] = true;
        }
        if (my_r > 0 && a.residue_index[r - 1] + 1 == a.residue_index[r]) {
            my_consec = true;
            if (my_s == SLOT_N && takes_part(a, r - 1, type_row(a.aa[r - 1]), SLOT_C)) {
                mine.x[2] = load_atom(a.pos + ((r - 1) * A + SLOT_C) * 3);
                mine.has[2] = true;
            }
        }
    }

    // the column tiles to visit, ascending: wave 0, a tile per lane
    if (tid < 64) {
        int rc = -1, best = 2 * TR;                         // the row residue nearest the tile's middle
        for (int r = r0; r < r1; ++r) {
            const int off = 2 * (r - r0) - (TR - 1), dist = off < 0 ? -off : off;
            if (work[r].w >= 0.f && (!query || query[r]) && dist < best) {
                best = dist;
                rc = r;
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
                keep = keep || (w.w >= 0.f && dist3(w, C) <= ((E + w.w) + reach) * CULL_SLACK);
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
    const bool my_d = (me.flg & DONOR) != 0, my_a = (me.flg & ACCEPTOR) != 0;
    const bool my_cat = (me.flg & CATION) != 0, my_an = (me.flg & ANION) != 0;
    const bool my_o = my_s == SLOT_O || my_s == SLOT_OXT;

    int n_hb = 0, n_sb = 0, n_hb_x = 0, n_sb_x = 0;
    int hb_list[K], sb_list[K];
#pragma unroll
    for (int k = 0; k < K; ++k) hb_list[k] = sb_list[k] = -1;

    if (cnt > 0) {
        commit_tile(tile[0], fetch_tile(a, b, list[0], tid, -FAR), tid);
        __syncthreads();
    }
    for (int k = 0; k < cnt; ++k) {
        Fetched next;
        const bool more = k + 1 < cnt;
        if (more) next = fetch_tile(a, b, list[k + 1], tid, -FAR);
        const Tile& T = tile[k & 1];
        const int q0 = list[k] * TR;
        for (int c = 0; c < TR; ++c) {
            const int q = q0 + c;
            const bool other_res = q != my_r;
            const bool other_grp = T.grp[c] != my_grp;
            for (int s = 0; s < SL; ++s) {
                const float4 v = T.a[c * SL + s];
                const float dx = P.x - v.x, dy = P.y - v.y, dz = P.z - v.z;
                const float r2 = (dx * dx + dy * dy) + dz * dz;
                if (other_res && r2 <= cut2) {
                    const unsigned char f = T.flg[c * SL + s];
                    const bool can_da = my_d && (f & ACCEPTOR), can_ad = my_a && (f & DONOR);
                    // the 1-3 pair: N of a residue with O / OXT of the chain-consecutive residue before it
                    const bool excluded = (my_s == SLOT_N && my_consec && q == my_r - 1 && (s == SLOT_O || s == SLOT_OXT)) ||
                                          (s == SLOT_N && T.consec[c] && my_r == q - 1 && my_o);
                    bool hb = false;
                    if ((can_da || can_ad) && r2 <= dmax2 && !excluded) {
                        Ants its;
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const int t = T.ant[c * SL + s][j];
                            its.has[j] = t >= 0;
                            its.x[j] = T.a[c * SL + (t >= 0 ? t : 0)];
                        }
                        its.x[2] = T.prev_c[c];
                        its.has[2] = s == SLOT_N && its.x[2].w != 0.f;
                        if (can_da) hb = angles_ok(P, mine, v, its, cos_acc, cos_don);
                        if (!hb && can_ad) hb = angles_ok(v, its, P, mine, cos_acc, cos_don);
                    }
                    const bool sb = r2 <= salt2 && ((my_cat && (f & ANION)) || (my_an && (f & CATION)));
                    const int flat = q * SL + s;
                    if (hb) {
#pragma unroll
                        for (int j = 0; j < K; ++j)
                            if (n_hb == j) hb_list[j] = flat;
                        n_hb += 1;
                        n_hb_x += other_grp;
                    }
                    if (sb) {
#pragma unroll
                        for (int j = 0; j < K; ++j)
                            if (n_sb == j) sb_list[j] = flat;
                        n_sb += 1;
                        n_sb_x += other_grp;
                    }
                }
            }
        }
        if (more) commit_tile(tile[(k + 1) & 1], next, tid);
        __syncthreads();
    }

    if (tid < TA) {
        red[0][tid] = n_hb;
        red[1][tid] = n_sb;
        red[2][tid] = n_hb_x;
        red[3][tid] = n_sb_x;
        if (my_r < N) {
            const size_t o = (b * N + my_r) * SL + my_s;
            const bool skipped = me.exists && !is_row;
            a.hbonds_atom[o] = skipped ? -1 : n_hb;
            a.salt_atom[o] = skipped ? -1 : n_sb;
            if (grouped) {
                a.hbonds_atom_cross[o] = skipped ? -1 : n_hb_x;
                a.salt_atom_cross[o] = skipped ? -1 : n_sb_x;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                a.hbond_partner[o * K + j] = hb_list[j];
                a.salt_partner[o * K + j] = sb_list[j];
            }
        }
    }
    __syncthreads();
    if (tid < TR && r0 + tid < N) {
        int s[4];
        for (int k = 0; k < 4; ++k) {
            s[k] = 0;
            for (int t = 0; t < SL; ++t) s[k] += red[k][tid * SL + t];
        }
        const size_t o = b * N + r0 + tid;
        a.hbonds_residue[o] = s[0];
        a.salt_residue[o] = s[1];
        if (grouped) {
            a.hbonds_residue_cross[o] = s[2];
            a.salt_residue_cross[o] = s[3];
        }
    }
}

__host__ inline bool positive_f(float v) { return v > 0.f && v < 1e6f; }
__host__ inline bool cosine_f(float v) { return v >= -1.f && v <= 1.f; }

}  // namespace

extern "C" int pf_polar_fwd(const pf_polar_args* a, pf_stream_t stream) {
    if (!a || !a->pos || !a->atom_mask || !a->aa || !a->residue_index || !a->types || !a->charge || !a->antecedents || !a->work ||
        !a->hbonds_atom || !a->salt_atom || !a->hbond_partner || !a->salt_partner || !a->hbonds_residue || !a->salt_residue)
        return PF_E_BADARG;
    const int n_cross = (a->hbonds_atom_cross != nullptr) + (a->salt_atom_cross != nullptr) + (a->hbonds_residue_cross != nullptr) +
                        (a->salt_residue_cross != nullptr);
    if ((a->group != nullptr) != (n_cross == 4) || (n_cross != 0 && n_cross != 4)) return PF_E_BADARG;
    if (a->B < 0 || a->N < 0 || a->N > PF_POLAR_MAX_N || a->n_atoms < SL - 1 || !positive_f(a->d_max) || !positive_f(a->salt_max) ||
        !cosine_f(a->cos_acc) || !cosine_f(a->cos_don))
        return PF_E_BADARG;
    if (a->B > 65535) return PF_E_TOOLARGE;
    if (a->B == 0 || a->N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)a->B * a->N;
    hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, *a);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(polar_kernel, dim3((unsigned)((a->N + TR - 1) / TR), (unsigned)a->B), dim3(NT), 0, st, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
