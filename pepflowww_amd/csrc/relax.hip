// pf_relax_energy_fwd / pf_relax_fwd -- a restraint force field over the heavy atoms of a batch of structures, with its analytic
// gradient, and a monotone steepest-descent minimiser around it: the step between finding clashes (pf_violations_fwd) and scoring an
// interface (pf_interface_energy_fwd).  It is NOT Amber (openfold/np/relax/amber_minimize.py) and NOT Rosetta's FastRelax: there are
// no hydrogens, no electrostatics, no torsion terms and no fitted parameter.  The terms are the clash overlap and the peptide-bond
// ideals of csrc/violations.hip plus the reference structure's own internal distances; it replaces those programs in role only, not
// in values.  Checked against the float64 restatement tests/relax_oracle.py and hand-computed minima.
//
// Conventions (tests/relax_oracle.py restates them in numpy):
//   Atoms     slots 0 .. min(n_atoms, 15) - 1 of pos [B,N,n_atoms,3] in the package's heavy-atom order (slot 14 is OXT), n_atoms >= 14.
//             An atom exists where atom_mask is set and radius [21,15] (geometry.sasa_radius_table: C 1.7, N 1.55, O 1.52, S 1.8) has
//             a non-zero entry for the residue's type row (a type outside 0..19 reads row 20) and the slot.  The existing atoms of
//             movable residues move; every other atom is a fixed partner.  ref_pos: same shape as pos.
//   E         = E_rest + E_intra + E_conn + E_clash, every term in fp32 per atom (or connection), the per-sample sums in float64.
//   E_rest    1/2 k_rest sum |x - x_ref|^2 over moving atoms.
//   E_intra   1/2 k_intra sum (|x_a - x_b| - |xref_a - xref_b|)^2 over the restrained pairs a < b of each movable residue, both atoms
//             existing; pair_mask [21,15]: bit b of (type row, a) (geometry.restrained_pair_table: at most two bonds apart, or in the
//             same rigid group -- bonds, angles and rings stay, psi and chi1-4 are free).  The gradient of |x_a - x_b| at 0 is 0.
//   E_conn    connection n = (n, n + 1) where residue_index[n + 1] - residue_index[n] == 1 and n or n + 1 is movable:
//             1/2 k_bond (|C_n - N_n+1| - l0)^2 where both exist, l0 = 1.329 (1.341 when n + 1 is a proline);
//             + 1/2 k_angle (cos(CA_n, C_n, N_n+1) + 0.4473)^2 where CA_n exists too; + 1/2 k_angle (cos(C_n, N_n+1, CA_n+1) + 0.5203)^2
//             where CA_n+1 exists too.  A term with a zero-length arm is left out.  The gradient goes to moving atoms only.
//   E_clash   1/2 k_clash sum relu(r_a + r_b - clash_overlap_tolerance + clash_margin - d)^2, d = sqrt(1e-10 + |x_a - x_b|^2), over
//             unordered pairs of existing atoms of different residue_index, at least one in a movable residue; excluded, as in
//             violations.hip: slot 2 (C) of index r with slot 0 (N) of index r + 1, and slot 5 with slot 5.
//   Per atom  terms_atom [B,N,15,4] (rest, intra, conn, clash) counts every pair and connection once over the atoms: an intra pair and
//             a clash between two moving atoms give half to each, a clash with a fixed partner goes to the moving atom, connection n
//             goes to C_n if n is movable and to N_n+1 otherwise.  energy_atom = ((rest + intra) + conn) + clash.  gradient [B,N,15,3]
//             = ((rest + intra) + conn) + clash, the full dE/dx of the atom; zero on atoms that do not move.
//   Sums      terms [B,4]: float64, thread t of 256 adds atoms t, t + 256, ... in ascending order, then a tree over the threads;
//             energy = ((rest + intra) + conn) + clash.
//   Minimiser accepted state (x, E, g, alpha), alpha = step0.  Iteration i = 1 .. steps: trial y = x - alpha g (fp32, moving atoms);
//             accepted when E(y) <= E in the float64 sums (then alpha <- min(1.2f alpha, 1000)), else x stays and alpha <- 0.5f alpha.
//             The cap keeps alpha finite however long a run accepts, so alpha g stays 0 on atoms that do not move.
//             energy_trace[i] = the accepted energy after iteration i (energy_trace[0]: the input's), accepted[i - 1], step_size[i - 1]
//             = the alpha of trial i.  After an acceptance (or at the start) with max|g| <= gtol the sample is frozen: later
//             iterations record accepted = 0, the same energy and the same alpha, and launch no work; iterations = the iterations run.
//
// No atomics, nothing pair-sized, one writer per output, every sum in a fixed order (column tiles ascending, the atoms of a tile
// ascending; only overlapping pairs are added, and adding nothing is exact, so culling does not show): bit-identical from run to run,
// independent of the rest of the batch and of its order.  Decisions are taken on the device; the host reads nothing back in the loop.
//   init_kernel   a thread per residue: work [B,N,4] = (centre, extent): its CA (or first existing atom) and the largest (distance
//                 from it + radius) of an existing atom (-1: none); for pf_relax_fwd also x = y = pos (slots 0..14), g = 0.
//   grad_kernel   grid (row tiles of 16 residues, B), 256 threads; thread t < 240 owns row atom (t / 15, t % 15) and is the sole writer
//                 of its gradient and partial energies.  A tile without a movable residue writes zeros and leaves, as does every tile
//                 of a frozen sample (without writing).  Column tiles are staged in LDS as float4 (x, y, z, radius; 0: no atom) plus
//                 residue_index and flags per residue, double-buffered; all lanes of a wave read the SAME column atom in a step (a
//                 broadcast, no bank conflict).  Wave 0 lists the column tiles to visit, a tile per lane: those with a residue whose
//                 sphere comes within (clash_margin - clash_overlap_tolerance) of the sphere round the tile's movable residues; the
//                 radii are inside the extents, so the reach is < 2.3 A (the share of tiles this drops: NOTES.md section 13).  The row tile itself and its
//                 reference are staged once for the intra term; the connection terms read their four atoms from global memory.
//   step_kernel   one workgroup per sample: sums the partial energies, decides, copies (x, g) on acceptance, updates alpha, writes
//                 the trace, the next trial y and the bounds of the movable residues at y.  Each iteration: grad_kernel + step_kernel.
//
// Replay tolerance (tests/test_gpu_relax.py::test_replay): 40 iterations from the clashing case, final positions against the float64
// oracle replaying the device's decisions: 4 x (oracle in fp32 against float64, 3.0e-6 A) = 1.2e-5 A; the device was 3.0e-6 A from the oracle.
#include "common.h"
#include "../../include/pepflow_hip.h"
#include "eval_dev.h"

namespace {

constexpr int TR = 16, SL = PF_RELAX_SLOTS, TA = TR * SL;       // residues per tile, slots per residue, atoms per tile
constexpr int NT = 256;
constexpr int MAX_TILES = PF_RELAX_MAX_N / TR;
constexpr int NE = PF_RELAX_TERMS;
constexpr unsigned char F_VALID = 1, F_MOV = 2;
constexpr float CN_LEN = 1.329f, CN_LEN_PRO = 1.341f, COS_CA_C_N = -0.4473f, COS_C_N_CA = -0.5203f;
constexpr float CLASH_EPS = 1e-10f;
constexpr float ALPHA_MAX = 1e3f;                       // the step size never grows beyond this (1.2^n would overflow after ~490 acceptances)

struct Tile {
    float4 at[TA];                  // x, y, z, radius (0: no atom)
    int idx[TR];
    unsigned char flg[TR];
};

struct Fetched {
    float4 at;
    int idx;
    unsigned char flg;
};

__device__ __forceinline__ float dot3(const float u[3], const float v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__device__ __forceinline__ float dist3(const float4& p, const float4& q) {
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// atom s of residue r = b N + q exists (s < 15)
__device__ __forceinline__ bool atom_exists(const pf_relax_args& a, size_t r, int s) {
    return s < a.n_atoms && a.atom_mask[r * a.n_atoms + s] != 0 && a.radius[type_row(a.aa[r]) * SL + s] > 0.f;
}

// (centre, extent) of residue r at positions P (atom stride PA): its CA if it exists, else its first existing atom, and the largest
// (distance + radius) of an existing atom; w = -1: no atom
__device__ __forceinline__ float4 residue_bounds(const pf_relax_args& a, const float* P, int PA, size_t r) {
    const int S = a.n_atoms < SL ? a.n_atoms : SL;
    const float* p = P + r * PA * 3;
    const unsigned char* m = a.atom_mask + r * a.n_atoms;
    const float* rad = a.radius + type_row(a.aa[r]) * SL;
    int c = -1;
    if (m[1] && rad[1] > 0.f) c = 1;
    for (int s = 0; s < S && c < 0; ++s)
        if (m[s] && rad[s] > 0.f) c = s;
    float4 w = make_float4(0.f, 0.f, 0.f, -1.f);
    if (c >= 0) {
        w = make_float4(p[3 * c], p[3 * c + 1], p[3 * c + 2], 0.f);
        for (int s = 0; s < S; ++s)
            if (m[s] && rad[s] > 0.f) w.w = fmaxf(w.w, dist3(make_float4(p[3 * s], p[3 * s + 1], p[3 * s + 2], 0.f), w) + rad[s]);
    }
    return w;
}

__global__ __launch_bounds__(256) void init_kernel(pf_relax_args a, int state) {
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= (size_t)a.B * a.N) return;
    reinterpret_cast<float4*>(a.work)[r] = residue_bounds(a, a.pos, a.n_atoms, r);
    if (!state) return;
    const int A = a.n_atoms;
    for (int s = 0; s < SL; ++s)
        for (int k = 0; k < 3; ++k) {
            const float v = s < A ? a.pos[(r * A + s) * 3 + k] : 0.f;
            const size_t o = (r * SL + s) * 3 + k;
            a.x[o] = v;
            a.y[o] = v;
            a.g[o] = 0.f;
        }
}

// thread t < 240: atom t of column tile ct of sample b at positions P; thread t < 16: residue t of it.  Addresses are formed only for
// q < N, s < n_atoms.
__device__ __forceinline__ Fetched fetch_tile(const pf_relax_args& a, const float* P, int PA, size_t b, int ct, int tid) {
    Fetched f;
    f.at = make_float4(0.f, 0.f, 0.f, 0.f);
    f.idx = 0;
    f.flg = 0;
    const int N = a.N;
    if (tid < TA) {
        const int q = ct * TR + tid / SL, s = tid % SL;
        if (q < N && s < a.n_atoms) {
            const size_t r = b * N + q;
            const float rad = a.radius[type_row(a.aa[r]) * SL + s];
            if (a.atom_mask[r * a.n_atoms + s] != 0 && rad > 0.f) {
                const float* p = P + (r * PA + s) * 3;
                f.at = make_float4(p[0], p[1], p[2], rad);
            }
        }
    }
    if (tid < TR) {
        const int q = ct * TR + tid;
        if (q < N) {
            f.idx = a.residue_index[b * N + q];
            f.flg = (unsigned char)(F_VALID | (a.movable[b * N + q] ? F_MOV : 0));
        }
    }
    return f;
}

__device__ __forceinline__ void commit_tile(Tile& t, const Fetched& f, int tid) {
    if (tid < TA) t.at[tid] = f.at;
    if (tid < TR) {
        t.idx[tid] = f.idx;
        t.flg[tid] = f.flg;
    }
}

struct Conn {
    float e;
    float g[4][3];                  // dE/d(CA_n, C_n, N_n+1, CA_n+1)
};

// connection (n, n + 1) of sample b at positions P, 0 <= n < N - 1
__device__ __forceinline__ Conn connection(const pf_relax_args& a, const float* P, int PA, size_t b, int n) {
    Conn o;
    o.e = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) o.g[i][0] = o.g[i][1] = o.g[i][2] = 0.f;
    const size_t r0 = b * a.N + n, r1 = r0 + 1;
    if ((long long)a.residue_index[r1] - (long long)a.residue_index[r0] != 1 || !(a.movable[r0] || a.movable[r1])) return o;
    if (!atom_exists(a, r0, 2) || !atom_exists(a, r1, 0)) return o;
    const float* P0 = P + r0 * PA * 3;
    const float* P1 = P + r1 * PA * 3;
    float u[3], v[3], w[3];                                 // CA_n - C_n, N_n+1 - C_n, CA_n+1 - N_n+1
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u[k] = P0[3 + k] - P0[6 + k];
        v[k] = P1[k] - P0[6 + k];
        w[k] = P1[3 + k] - P1[k];
    }
    const float lv = sqrtf(dot3(v, v));
    if (!(lv > 0.f)) return o;
    const float l0 = a.aa[r1] == a.pro ? CN_LEN_PRO : CN_LEN;
    const float dl = lv - l0;
    o.e = (0.5f * a.k_bond) * (dl * dl);
    const float fb = a.k_bond * dl;
    float vh[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vh[k] = v[k] / lv;
        o.g[2][k] = fb * vh[k];
        o.g[1][k] = -(fb * vh[k]);
    }
    const float lu = sqrtf(dot3(u, u));
    if (atom_exists(a, r0, 1) && lu > 0.f) {
        float uh[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) uh[k] = u[k] / lu;
        const float c = dot3(uh, vh), dc = c - COS_CA_C_N, f = a.k_angle * dc;
        o.e += (0.5f * a.k_angle) * (dc * dc);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float d_ca = (vh[k] - c * uh[k]) / lu, d_n = (uh[k] - c * vh[k]) / lv;
            o.g[0][k] += f * d_ca;
            o.g[2][k] += f * d_n;
            o.g[1][k] -= f * (d_ca + d_n);
        }
    }
    const float lw = sqrtf(dot3(w, w));
    if (atom_exists(a, r1, 1) && lw > 0.f) {
        float wh[3], ph[3];                                 // ph: N_n+1 -> C_n
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            wh[k] = w[k] / lw;
            ph[k] = -vh[k];
        }
        const float c = dot3(ph, wh), dc = c - COS_C_N_CA, f = a.k_angle * dc;
        o.e += (0.5f * a.k_angle) * (dc * dc);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float d_c = (wh[k] - c * ph[k]) / lv, d_ca = (ph[k] - c * wh[k]) / lw;
            o.g[1][k] += f * d_c;
            o.g[3][k] += f * d_ca;
            o.g[2][k] -= f * (d_c + d_ca);
        }
    }
    return o;
}

// positions P [B,N,PA,3]: a.pos (PA = n_atoms) or the trial a.y (PA = 15); loop: a launch of pf_relax_fwd's loop (frozen samples leave)
__global__ __launch_bounds__(NT) void grad_kernel(pf_relax_args a, const float* P, int PA, int loop) {
    __shared__ Tile tile[2];
    __shared__ float4 own[TA], ref[TA];                     // the row tile and its reference; w = 1: the atom exists
    __shared__ int list[MAX_TILES];
    __shared__ int n_list;
    const int N = a.N, tid = threadIdx.x;
    const size_t b = blockIdx.y;
    if (loop && a.frozen[b]) return;
    const int rt = blockIdx.x, n_tiles = (N + TR - 1) / TR;
    const int r0 = rt * TR, r1 = r0 + TR < N ? r0 + TR : N;
    const unsigned char* movable = a.movable + b * N;
    const float4* work = reinterpret_cast<const float4*>(a.work) + b * N;

    // the thread's row atom
    const int q = r0 + tid / SL, s = tid % SL;
    const bool row = tid < TA && q < N;
    const size_t r = b * N + (row ? q : r0);
    float4 X = make_float4(0.f, 0.f, 0.f, 0.f), R = X;      // w: radius (0: no atom) / exists
    int idx_p = 0, pm = 0;
    bool moving = false;
    if (row && s < a.n_atoms) {
        const int tr = type_row(a.aa[r]);
        const float rad = a.radius[tr * SL + s];
        if (a.atom_mask[r * a.n_atoms + s] != 0 && rad > 0.f) {
            const float* p = P + (r * PA + s) * 3;
            const float* pr = a.ref_pos + (r * a.n_atoms + s) * 3;
            X = make_float4(p[0], p[1], p[2], rad);
            R = make_float4(pr[0], pr[1], pr[2], 1.f);
            moving = movable[q] != 0;
            pm = a.pair_mask[tr * SL + s];
        }
        idx_p = a.residue_index[r];
    }
    if (tid < TA) {
        own[tid] = X;
        ref[tid] = R;
    }
    const bool any_moving = __syncthreads_or(moving);       // (also the barrier behind own / ref)
    if (!any_moving) {
        if (row) {
            const size_t o = r * SL + s;
            a.gradient[o * 3] = a.gradient[o * 3 + 1] = a.gradient[o * 3 + 2] = 0.f;
            for (int k = 0; k < NE; ++k) a.terms_atom[o * NE + k] = 0.f;
            if (a.energy_atom) a.energy_atom[o] = 0.f;
        }
        return;
    }

    // the column tiles to visit, ascending: wave 0, a tile per lane
    if (tid < 64) {
        int rc = -1, best = 2 * TR;                         // the movable row residue nearest the tile's middle
        for (int p = r0; p < r1; ++p) {
            const int off = 2 * (p - r0) - (TR - 1), dist = off < 0 ? -off : off;
            if (work[p].w >= 0.f && movable[p] && dist < best) {
                best = dist;
                rc = p;
            }
        }
        bool keep = false;
        if (rc >= 0 && tid < n_tiles) {                     // (rc is the same in every lane)
            const float4 C = work[rc];
            float E = 0.f;
            for (int p = r0; p < r1; ++p) {
                const float4 w = work[p];
                if (w.w >= 0.f && movable[p]) E = fmaxf(E, dist3(w, C) + w.w);
            }
            const float reach = a.clash_margin - a.clash_overlap_tolerance;
            const int q1 = tid * TR + TR < N ? tid * TR + TR : N;
            for (int p = tid * TR; p < q1; ++p) {
                const float4 w = work[p];
                const float d = dist3(w, C), lim = (E + w.w) + reach;
                keep = keep || (w.w >= 0.f && d <= lim + (1e-4f * ((d + E) + w.w) + 1e-3f));
            }
        }
        const unsigned long long bal = __ballot(keep);
        if (keep) list[__popcll(bal & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) n_list = __popcll(bal);
    }
    __syncthreads();
    const int cnt = n_list;

    // clashes: s_cl = sum of w o^2, acc = sum of (o / d) (x_a - x_b)
    const float tol = a.clash_overlap_tolerance, margin = a.clash_margin;
    float s_cl = 0.f, acc[3] = {0.f, 0.f, 0.f};
    if (cnt > 0) {
        commit_tile(tile[0], fetch_tile(a, P, PA, b, list[0], tid), tid);
        __syncthreads();
    }
    for (int k = 0; k < cnt; ++k) {
        Fetched next;
        const bool more = k + 1 < cnt;
        if (more) next = fetch_tile(a, P, PA, b, list[k + 1], tid);
        const Tile& T = tile[k & 1];
        if (moving) {
            for (int c = 0; c < TR; ++c) {
                const int idx_q = T.idx[c];
                const unsigned char f = T.flg[c];
                if (!(f & F_VALID) || idx_q == idx_p) continue;
                const float wgt = (f & F_MOV) ? 0.5f : 1.f;
                const bool cn_next = s == 2 && (long long)idx_p + 1 == idx_q;      // own C, N of the next index
                const bool cn_prev = s == 0 && (long long)idx_q + 1 == idx_p;      // own N, C of the previous index
#pragma unroll 5
                for (int t = 0; t < SL; ++t) {
                    const float4 v = T.at[c * SL + t];
                    if (!(v.w > 0.f) || (t == 5 && s == 5) || (t == 0 && cn_next) || (t == 2 && cn_prev)) continue;
                    const float lim = ((X.w + v.w) - tol) + margin;
                    const float dx = X.x - v.x, dy = X.y - v.y, dz = X.z - v.z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (lim > 0.f && d2 < lim * lim * 1.0001f) {                    // a superset of d < lim
                        const float d = sqrtf(CLASH_EPS + d2);
                        if (d < lim) {
                            const float o = lim - d, od = o / d;
                            s_cl += wgt * (o * o);
                            acc[0] += od * dx;
                            acc[1] += od * dy;
                            acc[2] += od * dz;
                        }
                    }
                }
            }
        }
        if (more) commit_tile(tile[(k + 1) & 1], next, tid);
        __syncthreads();
    }

    float e[NE] = {0.f, 0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f};
    if (moving) {
        // restraint
        const float dx[3] = {X.x - R.x, X.y - R.y, X.z - R.z};
        e[0] = (0.5f * a.k_rest) * dot3(dx, dx);
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = a.k_rest * dx[k];
        // internal distances: the restrained partners of the own residue, ascending
        const int base = (tid / SL) * SL;
        float s_in = 0.f, ain[3] = {0.f, 0.f, 0.f};
        for (int t = 0; t < SL; ++t) {
            const float4 v = own[base + t], vr = ref[base + t];
            if (!((pm >> t) & 1) || !(v.w > 0.f)) continue;
            const float u[3] = {X.x - v.x, X.y - v.y, X.z - v.z}, ur[3] = {R.x - vr.x, R.y - vr.y, R.z - vr.z};
            const float d = sqrtf(dot3(u, u)), d0 = sqrtf(dot3(ur, ur)), diff = d - d0;
            s_in += diff * diff;
            const float f = d > 0.f ? diff / d : 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) ain[k] += f * u[k];
        }
        e[1] = (0.25f * a.k_intra) * s_in;
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] += a.k_intra * ain[k];
        // connections: N takes part in n - 1, CA in n - 1 and n, C in n
        if (s <= 2) {
            float gc[3] = {0.f, 0.f, 0.f};
            if (s <= 1 && q > 0) {
                const Conn o = connection(a, P, PA, b, q - 1);
#pragma unroll
                for (int k = 0; k < 3; ++k) gc[k] = o.g[s == 0 ? 2 : 3][k];
                if (s == 0 && !movable[q - 1]) e[2] = o.e;
            }
            if (s >= 1 && q + 1 < N) {
                const Conn o = connection(a, P, PA, b, q);
#pragma unroll
                for (int k = 0; k < 3; ++k) gc[k] += o.g[s == 1 ? 0 : 1][k];
                if (s == 2) e[2] = o.e;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] += gc[k];
        }
        // clashes
        e[3] = (0.5f * a.k_clash) * s_cl;
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] += -(a.k_clash * acc[k]);
    }
    if (row) {
        const size_t o = r * SL + s;
#pragma unroll
        for (int k = 0; k < 3; ++k) a.gradient[o * 3 + k] = g[k];
#pragma unroll
        for (int k = 0; k < NE; ++k) a.terms_atom[o * NE + k] = e[k];
        if (a.energy_atom) a.energy_atom[o] = ((e[0] + e[1]) + e[2]) + e[3];
    }
}

// it = -1: the sums only (pf_relax_energy_fwd); it = 0: the input's evaluation becomes the accepted state; it = 1 .. steps: iteration it
__global__ __launch_bounds__(NT) void step_kernel(pf_relax_args a, int it) {
    __shared__ double red[NT];
    const int N = a.N, tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const size_t na = (size_t)N * SL;
    const int steps = a.steps;
    if (it > 0 && a.frozen[b]) {
        if (tid == 0) {
            a.energy_trace[b * (steps + 1) + it] = a.energy[b];
            a.accepted[b * steps + it - 1] = 0;
            if (it < steps) a.step_size[b * steps + it] = a.alpha[b];
        }
        return;
    }
    const double E_old = it > 0 ? a.energy[b] : 0.0;
    const float alpha = it > 0 ? a.alpha[b] : a.step0;

    double t[NE] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = tid; i < na; i += NT)
#pragma unroll
        for (int k = 0; k < NE; ++k) t[k] += (double)a.terms_atom[(b * na + i) * NE + k];
#pragma unroll
    for (int k = 0; k < NE; ++k) t[k] = block_sum<NT>(t[k], red, tid);
    const double E_new = ((t[0] + t[1]) + t[2]) + t[3];
    if (it < 0) {
        if (tid == 0) {
            for (int k = 0; k < NE; ++k) a.terms[b * NE + k] = t[k];
            a.energy[b] = E_new;
        }
        return;
    }

    const bool accept = it == 0 || E_new <= E_old;          // (a NaN energy is rejected)
    const float alpha_new = it == 0 ? alpha : accept ? fminf(1.2f * alpha, ALPHA_MAX) : 0.5f * alpha;
    bool frozen = false;
    float* x = a.x + b * na * 3;
    float* g = a.g + b * na * 3;
    float* y = a.y + b * na * 3;
    if (accept) {
        const float* gy = a.gradient + b * na * 3;
        double gmax = 0.0;
        for (size_t i = tid; i < na * 3; i += NT) {
            const float gi = gy[i];
            x[i] = y[i];
            g[i] = gi;
            gmax = fmax(gmax, (double)fabsf(gi));
        }
        __syncthreads();
        red[tid] = gmax;
        __syncthreads();
        for (int h = NT / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] = fmax(red[tid], red[tid + h]);
            __syncthreads();
        }
        gmax = red[0];
        frozen = (float)gmax <= a.gtol;
        if (tid == 0) {
            for (int k = 0; k < NE; ++k) a.terms[b * NE + k] = t[k];
            a.energy[b] = E_new;
            a.grad_max[b] = (float)gmax;
            if (it == 0)
                for (int k = 0; k < NE; ++k) a.terms_initial[b * NE + k] = t[k];
        }
    }
    if (tid == 0) {
        a.energy_trace[b * (steps + 1) + it] = accept ? E_new : E_old;
        if (it > 0) a.accepted[b * steps + it - 1] = accept;
        if (it < steps) a.step_size[b * steps + it] = alpha_new;
        a.alpha[b] = alpha_new;
        a.frozen[b] = frozen;
        a.iterations[b] = it;
    }
    if (it >= steps || frozen) return;

    // the next trial (a thread reads what it wrote above: the same indices), then the bounds of the movable residues at it
    for (size_t i = tid; i < na * 3; i += NT) y[i] = x[i] - alpha_new * g[i];
    __syncthreads();
    for (int n = tid; n < N; n += NT)
        if (a.movable[b * N + n]) reinterpret_cast<float4*>(a.work)[b * N + n] = residue_bounds(a, a.y, SL, b * N + n);
}

__host__ inline bool positive_f(float v) { return v > 0.f && v < 1e30f; }
__host__ inline bool finite_f(float v) { return v == v && v - v == 0.f; }

__host__ int check_args(const pf_relax_args* a, bool loop) {
    if (!a || !a->pos || !a->ref_pos || !a->atom_mask || !a->aa || !a->residue_index || !a->movable || !a->radius || !a->pair_mask ||
        !a->work || !a->gradient || !a->terms_atom || !a->terms || !a->energy || a->B < 0 || a->N < 0 || a->n_atoms < SL - 1 ||
        !positive_f(a->k_rest) || !positive_f(a->k_intra) || !positive_f(a->k_bond) || !positive_f(a->k_angle) ||
        !positive_f(a->k_clash) || !finite_f(a->clash_overlap_tolerance) || !finite_f(a->clash_margin))
        return PF_E_BADARG;
    if (loop && (!a->x || !a->g || !a->y || !a->alpha || !a->frozen || !a->terms_initial || !a->energy_trace || !a->grad_max ||
                 !a->iterations || a->steps < 0 || (a->steps > 0 && (!a->accepted || !a->step_size)) || !positive_f(a->step0) ||
                 !(a->gtol >= 0.f) || !finite_f(a->gtol)))
        return PF_E_BADARG;
    if (a->N > PF_RELAX_MAX_N || a->B > 65535) return PF_E_TOOLARGE;
    return 0;
}

}  // namespace

extern "C" int pf_relax_energy_fwd(const pf_relax_args* a, pf_stream_t stream) {
    if (const int rc = check_args(a, false)) return rc;
    if (a->B == 0 || a->N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)a->B * a->N;
    hipLaunchKernelGGL(init_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, *a, 0);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_kernel, dim3((unsigned)((a->N + TR - 1) / TR), (unsigned)a->B), dim3(NT), 0, st, *a, a->pos, a->n_atoms, 0);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(step_kernel, dim3((unsigned)a->B), dim3(NT), 0, st, *a, -1);
    PF_CHECK_LAUNCH();
    return 0;
}

extern "C" int pf_relax_fwd(const pf_relax_args* a, pf_stream_t stream) {
    if (const int rc = check_args(a, true)) return rc;
    if (a->B == 0 || a->N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)a->B * a->N;
    hipLaunchKernelGGL(init_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, *a, 1);
    PF_CHECK_LAUNCH();
    for (int it = 0; it <= a->steps; ++it) {
        hipLaunchKernelGGL(grad_kernel, dim3((unsigned)((a->N + TR - 1) / TR), (unsigned)a->B), dim3(NT), 0, st, *a, (const float*)a->y, SL,
                           it > 0);
        PF_CHECK_LAUNCH();
        hipLaunchKernelGGL(step_kernel, dim3((unsigned)a->B), dim3(NT), 0, st, *a, it);
        PF_CHECK_LAUNCH();
    }
    return 0;
}
