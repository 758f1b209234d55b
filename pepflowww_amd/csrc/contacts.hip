// pf_contacts_fwd -- residue-residue contacts across an interface in a model and in a reference structure at once: what DockQ's
// Fnat and its interface definition need (Basu & Wallner, PLoS ONE 2016).  Written from the publication; not checked against the
// DockQ program.
//
// Conventions (tests/lddt_oracle.py restates them in numpy):
//   Pair      pair p = (i, j) of pairs [P,2] looks at the model x[i] and the reference structure y[j]; group [By,N] belongs to y.  A
//             pair with an index out of range gives zero counts, no interface and +inf distances.
//   Atoms     slots 0 .. min(n_atoms, 15) - 1 whose bit is in slot_mask; an atom exists in a structure on that structure's OWN
//             atom_mask.  There is no residue-type rule: each structure's contacts are counted on the atoms it has.
//   Counted   a residue pair (p, q) counts when the two residues have different group bytes and each of them has at least one atom in
//             x[i] and at least one in y[j].  For it m_x = the minimal squared atom distance in x[i], m_y the same in y[j], in fp32,
//             compared as m < cutoff^2 (no square root).
//   Outputs   per row residue p, over the counted q: contacts_x, contacts_y, contacts_shared [P,N] int32 -- the q with
//             m_x < contact_cutoff^2, with m_y < contact_cutoff^2, with both; interface_x, interface_y [P,N] bytes -- some q with
//             m < interface_cutoff^2; min_dist_x, min_dist_y [P,N] fp32 -- sqrt of the smallest m over the counted q, +inf without any.
//             Each unordered residue pair shows in both of its rows: callers sum over one group.
//
// One launch, no atomics, no scratch, nothing pair-sized: integer counts, flags and minima with one writer each, so the results are
// bit-identical from run to run and depend neither on the rest of the batch nor on the order of the work list.
//   contacts_kernel   grid (row tiles of 16 residues, pairs), 256 threads, thread (t / 16, t % 16) owns the residue pair (row residue,
//                     column residue) of the current column tile and loops over its 15 x 15 atom pairs in both structures, without an
//                     early exit.  Tiles are staged in LDS as float4, 15 to a residue: 16 lanes of a ds_read_b128 group read 16
//                     column residues 15 float4 = 60 dwords apart, which fall into 16 different sets of four banks, and the two row
//                     residues of such a group are one odd stride apart as well (MI355X: 64 banks, groups of 16 lanes).  An atom that
//                     does not exist has x = +1e18 in a row tile and -1e18 in a column tile, so any pair with it is ~1e36 and no
//                     lane branches on a mask.  Column tiles are double-buffered; those without a residue of another group than the
//                     row tile's come off a list built in LDS.  The 16 column threads of a row residue are combined through LDS;
//                     column tiles accumulate in ascending order.
#include "common.h"
#include "../../include/pepflow_hip.h"

namespace {

constexpr int TR = 16, SL = PF_CONTACTS_SLOTS, TA = TR * SL;    // residues per tile, slots per residue, atoms per tile
constexpr int NT = 256;
constexpr int MAX_TILES = PF_CONTACTS_MAX_N / TR;
constexpr int MAX_PAIRS_PER_LAUNCH = 65535;
constexpr float FAR = 1e18f;
constexpr unsigned char HAS_X = 1, HAS_Y = 2, VALID = 4;

struct Tile {
    float4 x[TA];
    float4 y[TA];
    unsigned char grp[TR];
    unsigned char flg[TR];
};

struct Fetched {
    float4 x, y;
    unsigned char grp, flg;
};

__device__ __forceinline__ bool exists(const unsigned char* mask, size_t r, int n_atoms, int s, int slot_mask) {
    return s < n_atoms && ((slot_mask >> s) & 1) && mask[r * n_atoms + s] != 0;
}

// thread t < 240: atom t of tile ct of x[i] and y[j] (absent: x = far); thread t < 16: residue t of it.  Loads come from clamped
// (valid) addresses, and a coordinate is used only where the atom exists.
__device__ __forceinline__ Fetched fetch_tile(const pf_contacts_args& a, size_t i, size_t j, int ct, int tid, float far) {
    Fetched f;
    f.x = make_float4(far, 0.f, 0.f, 0.f);
    f.y = make_float4(far, 0.f, 0.f, 0.f);
    f.grp = 0;
    f.flg = 0;
    const int N = a.N;
    if (tid < TA) {
        const int q = ct * TR + tid / SL, s = tid % SL;
        if (q < N) {
            const size_t rx = i * N + q, ry = j * N + q;
            if (exists(a.mask_x, rx, a.n_atoms_x, s, a.slot_mask)) {
                const float* px = a.pos_x + (rx * a.n_atoms_x + s) * 3;
                f.x = make_float4(px[0], px[1], px[2], 0.f);
            }
            if (exists(a.mask_y, ry, a.n_atoms_y, s, a.slot_mask)) {
                const float* py = a.pos_y + (ry * a.n_atoms_y + s) * 3;
                f.y = make_float4(py[0], py[1], py[2], 0.f);
            }
        }
    }
    if (tid < TR) {
        const int q = ct * TR + tid;
        if (q < N) {
            const size_t rx = i * N + q, ry = j * N + q;
            bool hx = false, hy = false;
            for (int s = 0; s < SL; ++s) {
                hx = hx || exists(a.mask_x, rx, a.n_atoms_x, s, a.slot_mask);
                hy = hy || exists(a.mask_y, ry, a.n_atoms_y, s, a.slot_mask);
            }
            f.grp = a.group[ry];
            f.flg = (unsigned char)(VALID | (hx ? HAS_X : 0) | (hy ? HAS_Y : 0));
        }
    }
    return f;
}

__device__ __forceinline__ void commit_tile(Tile& t, const Fetched& f, int tid) {
    if (tid < TA) {
        t.x[tid] = f.x;
        t.y[tid] = f.y;
    }
    if (tid < TR) {
        t.grp[tid] = f.grp;
        t.flg[tid] = f.flg;
    }
}

// the minimal squared distance between the 15 atoms at r and the 15 at c
__device__ __forceinline__ float min_d2(const float4* r, const float4* c) {
    float cx[SL], cy[SL], cz[SL];
#pragma unroll
    for (int t = 0; t < SL; ++t) {
        const float4 v = c[t];
        cx[t] = v.x; cy[t] = v.y; cz[t] = v.z;
    }
    float m = __builtin_inff();
#pragma unroll
    for (int s = 0; s < SL; ++s) {
        const float4 v = r[s];
#pragma unroll
        for (int t = 0; t < SL; ++t) {
            const float dx = v.x - cx[t], dy = v.y - cy[t], dz = v.z - cz[t];
            m = fminf(m, (dx * dx + dy * dy) + dz * dz);
        }
    }
    return m;
}

__global__ __launch_bounds__(NT) void contacts_kernel(pf_contacts_args a, int p0) {
    __shared__ Tile rowt, tile[2];
    __shared__ int list[MAX_TILES];
    __shared__ int n_list;
    __shared__ int red_i[3][NT];
    __shared__ float red_f[2][NT];
    __shared__ unsigned char red_b[2][NT];
    const int N = a.N, tid = threadIdx.x;
    const size_t pp = (size_t)p0 + blockIdx.y;
    const int rt = blockIdx.x, n_tiles = (N + TR - 1) / TR;
    const int pi = a.pairs[2 * pp], pj = a.pairs[2 * pp + 1];
    const bool valid = pi >= 0 && pi < a.Bx && pj >= 0 && pj < a.By;        // uniform over the workgroup
    const size_t i = valid ? pi : 0, j = valid ? pj : 0;
    const float cc2 = a.contact_cutoff * a.contact_cutoff, ic2 = a.interface_cutoff * a.interface_cutoff;
    const int rr = tid / TR, cc = tid % TR;

    commit_tile(rowt, fetch_tile(a, i, j, rt, tid, FAR), tid);
    __syncthreads();

    // the column tiles that hold a residue of another group than one of the row tile's, ascending: wave 0, one tile per lane
    if (tid < 64) {
        int lo = 256, hi = -1;                              // the row tile's group bytes
        for (int r = 0; r < TR; ++r)
            if (rowt.flg[r] & VALID) {
                lo = min(lo, (int)rowt.grp[r]);
                hi = max(hi, (int)rowt.grp[r]);
            }
        bool work = valid && tid < n_tiles && hi >= 0;
        if (work && lo == hi) {
            work = false;
            const unsigned char* g = a.group + j * N;
            for (int q = tid * TR; q < min(N, tid * TR + TR); ++q) work = work || g[q] != lo;
        }
        const unsigned long long bal = __ballot(work);
        if (work) list[__popcll(bal & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) n_list = __popcll(bal);
    }
    __syncthreads();
    const int cnt = n_list;

    const unsigned char grp_p = rowt.grp[rr], flg_p = rowt.flg[rr];
    int n_x = 0, n_y = 0, n_s = 0;
    bool if_x = false, if_y = false;
    float mn_x = __builtin_inff(), mn_y = __builtin_inff();

    if (cnt > 0) {
        commit_tile(tile[0], fetch_tile(a, i, j, list[0], tid, -FAR), tid);
        __syncthreads();
    }
    for (int k = 0; k < cnt; ++k) {
        Fetched next;
        const bool more = k + 1 < cnt;
        if (more) next = fetch_tile(a, i, j, list[k + 1], tid, -FAR);
        const Tile& T = tile[k & 1];
        const float m_x = min_d2(rowt.x + rr * SL, T.x + cc * SL);
        const float m_y = min_d2(rowt.y + rr * SL, T.y + cc * SL);
        const unsigned char f = T.flg[cc] & flg_p;
        if (f == (VALID | HAS_X | HAS_Y) && T.grp[cc] != grp_p) {
            const bool cx = m_x < cc2, cy = m_y < cc2;
            n_x += cx;
            n_y += cy;
            n_s += cx && cy;
            if_x = if_x || m_x < ic2;
            if_y = if_y || m_y < ic2;
            mn_x = fminf(mn_x, m_x);
            mn_y = fminf(mn_y, m_y);
        }
        if (more) commit_tile(tile[(k + 1) & 1], next, tid);
        __syncthreads();
    }

    red_i[0][tid] = n_x;
    red_i[1][tid] = n_y;
    red_i[2][tid] = n_s;
    red_b[0][tid] = if_x;
    red_b[1][tid] = if_y;
    red_f[0][tid] = mn_x;
    red_f[1][tid] = mn_y;
    __syncthreads();
    if (tid < TR && rt * TR + tid < N) {
        int s0 = 0, s1 = 0, s2 = 0;
        bool b0 = false, b1 = false;
        float f0 = __builtin_inff(), f1 = __builtin_inff();
        for (int c = 0; c < TR; ++c) {
            const int e = tid * TR + c;
            s0 += red_i[0][e];
            s1 += red_i[1][e];
            s2 += red_i[2][e];
            b0 = b0 || red_b[0][e];
            b1 = b1 || red_b[1][e];
            f0 = fminf(f0, red_f[0][e]);
            f1 = fminf(f1, red_f[1][e]);
        }
        const size_t o = pp * N + rt * TR + tid;
        a.contacts_x[o] = s0;
        a.contacts_y[o] = s1;
        a.contacts_shared[o] = s2;
        a.interface_x[o] = b0;
        a.interface_y[o] = b1;
        a.min_dist_x[o] = sqrtf(f0);
        a.min_dist_y[o] = sqrtf(f1);
    }
}

}  // namespace

extern "C" int pf_contacts_fwd(const pf_contacts_args* a, pf_stream_t stream) {
    if (!a || !a->pos_x || !a->pos_y || !a->mask_x || !a->mask_y || !a->pairs || !a->group || !a->contacts_x || !a->contacts_y ||
        !a->contacts_shared || !a->interface_x || !a->interface_y || !a->min_dist_x || !a->min_dist_y || a->Bx < 1 || a->By < 1 ||
        a->N < 1 || a->P < 0 || a->n_atoms_x < 14 || a->n_atoms_y < 14 || !(a->contact_cutoff > 0.f) || !(a->contact_cutoff < 1e6f) ||
        !(a->interface_cutoff > 0.f) || !(a->interface_cutoff < 1e6f))
        return PF_E_BADARG;
    if (a->N > PF_CONTACTS_MAX_N) return PF_E_TOOLARGE;
    const unsigned tiles = (unsigned)((a->N + TR - 1) / TR);
    for (int p0 = 0; p0 < a->P; p0 += MAX_PAIRS_PER_LAUNCH) {
        const int np = a->P - p0 < MAX_PAIRS_PER_LAUNCH ? a->P - p0 : MAX_PAIRS_PER_LAUNCH;
        hipLaunchKernelGGL(contacts_kernel, dim3(tiles, (unsigned)np), dim3(NT), 0, (hipStream_t)stream, *a, p0);
        PF_CHECK_LAUNCH();
    }
    return 0;
}
