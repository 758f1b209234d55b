// pf_lddt_fwd -- the local distance difference test (lDDT; Mariani et al., Bioinformatics 2013) of a model against a reference
// structure, with the values of the reference's vendored OpenFold (openfold/utils/loss.py:382-458, `lddt` and `lddt_ca`): a
// superposition-free score over the atom pairs that are within `cutoff` in the reference structure.  The kernel returns integer
// counts; the score is kept / (4 scored), formed by the caller.
//
// Conventions (tests/lddt_oracle.py restates them in numpy):
//   Pair      pair p = (i, j) of pairs [P,2] compares the model x[i] with the reference structure y[j], residue n with residue n.
//             `group` and `query` [By,N] belong to y.  A pair with an index out of range gives zeros.
//   Atoms     slots 0..13 of pos [B,N,n_atoms,3] in the package's heavy-atom order; slots >= 14 (OXT) are never read.  An atom is
//             COMPARED when its slot is in slot_mask (bit s: slot s), it is set in mask_x[i] and in mask_y[j], and, for the side-chain
//             slots >= 4, aa_x[i] == aa_y[j] at that residue (a slot of two different residue types is not the same atom).
//   Distance  d = sqrt(1e-10 + |a - b|^2) in fp32, in each structure (loss.py:391-413).
//   Scored    a pair of compared atoms (a, b) is scored when d_y < cutoff, a and b are not the same atom and, with
//             exclude_same_residue, not in the same residue.  The reference scores pairs inside a residue (loss.py:414-419 removes the
//             diagonal only): exclude_same_residue = 0 is its behaviour; 1 gives the lDDT of Mariani et al.
//   Kept      a scored pair adds [|d_y - d_x| < 0.5] + [< 1] + [< 2] + [< 4] (loss.py:421-428).
//   Outputs   int32.  scored, kept [P,N]: per row residue, summed over the residue's atoms and all their partners; scored_atom,
//             kept_atom [P,N,14] per row atom; the *_cross forms keep only partners whose residue has another group byte.
//   query     only rows (atoms a) in query residues are evaluated, the rest are 0; every compared atom is still a partner b.
//
// One launch, no atomics, no scratch, nothing pair-sized and no floating-point sum: every output is an integer with one writer, so
// the results are bit-identical from run to run and depend neither on the rest of the batch nor on the order of the work list.
//   lddt_kernel   grid (row tiles of 16 residues, pairs), 256 threads, thread t < 224 owns atom (t / 14, t % 14) of the row tile in
//                 both structures.  Column tiles of 16 residues of both structures are staged in LDS as float4 (w of the x copy:
//                 compared) plus the group byte and a valid flag per residue, double-buffered, the next tile fetched into registers
//                 while the current one is evaluated; all lanes read the same LDS word (broadcast).  The per-residue sums go
//                 through LDS, slot by slot.  A row tile without an evaluated atom visits no column tile.
#include "common.h"
#include "../../include/pepflow_hip.h"

namespace {

constexpr int TR = 16, SL = PF_LDDT_SLOTS, TA = TR * SL;    // residues per tile, slots per residue, atoms per tile
constexpr int NT = 256;
constexpr int MAX_PAIRS_PER_LAUNCH = 65535;

struct Tile {
    float4 x[TA];           // w > 0: compared
    float4 y[TA];
    unsigned char grp[TR];
    unsigned char valid[TR];
};

struct Fetched {
    float4 x, y;
    unsigned char grp, valid;
};

__device__ __forceinline__ bool compared(const pf_lddt_args& a, size_t rx, size_t ry, int s) {
    return ((a.slot_mask >> s) & 1) && a.mask_x[rx * a.n_atoms_x + s] != 0 && a.mask_y[ry * a.n_atoms_y + s] != 0 &&
           (s < 4 || a.aa_x[rx] == a.aa_y[ry]);
}

// thread t < 224: atom t of column tile ct of x[i] and y[j]; thread t < 16: residue t of it.  Loads come from clamped (valid) addresses.
__device__ __forceinline__ Fetched fetch_tile(const pf_lddt_args& a, size_t i, size_t j, int ct, int tid) {
    Fetched f;
    f.x = make_float4(0.f, 0.f, 0.f, 0.f);
    f.y = make_float4(0.f, 0.f, 0.f, 0.f);
    f.grp = 0;
    f.valid = 0;
    const int N = a.N;
    if (tid < TA) {
        const int q = ct * TR + tid / SL, s = tid % SL;
        const int qc = q < N ? q : N - 1;
        const size_t rx = i * N + qc, ry = j * N + qc;
        const float* px = a.pos_x + (rx * a.n_atoms_x + s) * 3;
        const float* py = a.pos_y + (ry * a.n_atoms_y + s) * 3;
        const bool on = q < N && compared(a, rx, ry, s);
        f.x = make_float4(px[0], px[1], px[2], on ? 1.f : 0.f);
        f.y = make_float4(py[0], py[1], py[2], 0.f);
    }
    if (tid < TR) {
        const int q = ct * TR + tid;
        f.valid = q < N;
        f.grp = a.group ? a.group[j * N + (q < N ? q : N - 1)] : 0;
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
        t.valid[tid] = f.valid;
    }
}

__global__ __launch_bounds__(NT) void lddt_kernel(pf_lddt_args a, int p0) {
    __shared__ Tile tile[2];
    __shared__ int red[4][TA];
    const int N = a.N, tid = threadIdx.x;
    const size_t pp = (size_t)p0 + blockIdx.y;
    const int rt = blockIdx.x, n_tiles = (N + TR - 1) / TR;
    const int pi = a.pairs[2 * pp], pj = a.pairs[2 * pp + 1];
    const bool valid = pi >= 0 && pi < a.Bx && pj >= 0 && pj < a.By;        // uniform over the workgroup
    const size_t i = valid ? pi : 0, j = valid ? pj : 0;
    const float cutoff = a.cutoff, c2hi = cutoff * cutoff * 1.0001f;         // d2 < c2hi: a superset of d < cutoff
    const bool excl = a.exclude_same_residue != 0, has_group = a.group != nullptr;

    // the thread's own atom, in both structures
    const int p = rt * TR + tid / SL, s = tid % SL;
    const bool row = tid < TA && p < N;
    float ox = 0.f, oy = 0.f, oz = 0.f, rx_ = 0.f, ry_ = 0.f, rz_ = 0.f;     // own atom in x (o.) and in y (r.)
    bool on = false;
    unsigned char grp_p = 0;
    if (row && valid) {
        const size_t rx = i * N + p, ry = j * N + p;
        const float* px = a.pos_x + (rx * a.n_atoms_x + s) * 3;
        const float* py = a.pos_y + (ry * a.n_atoms_y + s) * 3;
        ox = px[0]; oy = px[1]; oz = px[2];
        rx_ = py[0]; ry_ = py[1]; rz_ = py[2];
        on = compared(a, rx, ry, s) && (!a.query || a.query[ry] != 0);
        grp_p = has_group ? a.group[ry] : 0;
    }
    const bool any_on = __syncthreads_or(on);

    int scored = 0, kept = 0, scored_c = 0, kept_c = 0;
    if (any_on) {
        commit_tile(tile[0], fetch_tile(a, i, j, 0, tid), tid);
        __syncthreads();
        for (int ct = 0; ct < n_tiles; ++ct) {
            Fetched next;
            const bool more = ct + 1 < n_tiles;
            if (more) next = fetch_tile(a, i, j, ct + 1, tid);
            const Tile& T = tile[ct & 1];
            if (on) {
                for (int r = 0; r < TR; ++r) {
                    if (!T.valid[r]) continue;
                    const bool same_res = ct * TR + r == p;
                    if (excl && same_res) continue;
                    const bool cross = has_group && T.grp[r] != grp_p;
#pragma unroll
                    for (int t = 0; t < SL; ++t) {
                        const float4 cx = T.x[r * SL + t];
                        if (!(cx.w > 0.f) || (same_res && t == s)) continue;
                        const float4 cy = T.y[r * SL + t];
                        const float ex = rx_ - cy.x, ey = ry_ - cy.y, ez = rz_ - cy.z;
                        const float d2y = (ex * ex + ey * ey) + ez * ez;
                        if (d2y < c2hi) {
                            const float dy = sqrtf(1e-10f + d2y);
                            if (dy < cutoff) {
                                const float fx = ox - cx.x, fy = oy - cx.y, fz = oz - cx.z;
                                const float dx = sqrtf(1e-10f + ((fx * fx + fy * fy) + fz * fz));
                                const float l1 = fabsf(dy - dx);
                                const int k = (int)(l1 < 0.5f) + (int)(l1 < 1.0f) + (int)(l1 < 2.0f) + (int)(l1 < 4.0f);
                                ++scored;
                                kept += k;
                                if (cross) {
                                    ++scored_c;
                                    kept_c += k;
                                }
                            }
                        }
                    }
                }
            }
            if (more) commit_tile(tile[(ct + 1) & 1], next, tid);
            __syncthreads();
        }
    }

    if (tid < TA) {
        red[0][tid] = scored;
        red[1][tid] = kept;
        red[2][tid] = scored_c;
        red[3][tid] = kept_c;
    }
    __syncthreads();
    if (row) {
        const size_t o = (pp * N + p) * SL + s;
        if (a.scored_atom) {
            a.scored_atom[o] = scored;
            a.kept_atom[o] = kept;
        }
        if (a.scored_atom_cross) {
            a.scored_atom_cross[o] = scored_c;
            a.kept_atom_cross[o] = kept_c;
        }
    }
    if (tid < TR && rt * TR + tid < N) {
        int sum[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            for (int t = 0; t < SL; ++t) sum[k] += red[k][tid * SL + t];
        const size_t o = pp * N + rt * TR + tid;
        a.scored[o] = sum[0];
        a.kept[o] = sum[1];
        if (a.scored_cross) {
            a.scored_cross[o] = sum[2];
            a.kept_cross[o] = sum[3];
        }
    }
}

}  // namespace

extern "C" int pf_lddt_fwd(const pf_lddt_args* a, pf_stream_t stream) {
    if (!a || !a->pos_x || !a->pos_y || !a->mask_x || !a->mask_y || !a->aa_x || !a->aa_y || !a->pairs || !a->scored || !a->kept ||
        a->Bx < 1 || a->By < 1 || a->N < 1 || a->P < 0 || a->n_atoms_x < SL || a->n_atoms_y < SL ||
        (!a->scored_cross != !a->kept_cross) || (!a->scored_atom != !a->kept_atom) || (!a->scored_atom_cross != !a->kept_atom_cross) ||
        ((a->scored_cross || a->scored_atom_cross) && !a->group) || !(a->cutoff > 0.f) || !(a->cutoff < 1e6f))
        return PF_E_BADARG;
    if (a->N > PF_LDDT_MAX_N) return PF_E_TOOLARGE;
    const unsigned tiles = (unsigned)((a->N + TR - 1) / TR);
    for (int p0 = 0; p0 < a->P; p0 += MAX_PAIRS_PER_LAUNCH) {
        const int np = a->P - p0 < MAX_PAIRS_PER_LAUNCH ? a->P - p0 : MAX_PAIRS_PER_LAUNCH;
        hipLaunchKernelGGL(lddt_kernel, dim3(tiles, (unsigned)np), dim3(NT), 0, (hipStream_t)stream, *a, p0);
        PF_CHECK_LAUNCH();
    }
    return 0;
}
