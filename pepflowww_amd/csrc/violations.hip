// pf_violations_fwd -- AlphaFold's between-residue structural violations (Jumper et al. 2021, Suppl. 1.9.11) of a batch of
// heavy-atom structures: steric clashes between residues and the geometry of the peptide bond between neighbours, with the values
// of the reference's vendored OpenFold (openfold/utils/loss.py): between_residue_clash_loss 871-1015, between_residue_bond_loss
// 712-868, extreme_ca_ca_distance_violations 1235-1269.  The within-residue part (1018-1102) is not computed.
//
// Conventions (tests/violation_oracle.py restates them in numpy):
//   Atoms     slots 0..13 of pos [B,N,n_atoms,3] in the package's heavy-atom order (N, CA, C, O, CB, ...: the same names in the same
//             order as OpenFold's atom14 for all 20 types); slots >= 14 (OXT) are not read.  An atom exists where atom_mask is set and
//             the radius table has an entry; radius [21,14] is indexed by the package's residue type (a type outside 0..19 reads
//             row 20) and the slot: C 1.7, N 1.55, O 1.52, S 1.8 (loss.py:1127-1135, residue_constants.py van_der_waals_radius).
//   Clash     a pair of atoms is counted when both exist, their residue_index differ (loss.py:930-933 keeps index_i < index_j, so
//             residues of EQUAL index -- the same residue, or two chains numbered alike -- are never compared), it is not slot 2 (C)
//             of index r with slot 0 (N) of index r + 1 (951-959), and it is not slot 5 with slot 5: the reference's disulfide
//             exclusion is a one-hot on slot 5 (CYS SG) applied to EVERY residue type (962-973), kept as it is.
//             d = sqrt(1e-10 + |x_a - x_b|^2), e = relu(r_a + r_b - tol - d), flag d < r_a + r_b - tol, in fp32.
//             clash_atom_loss = sum of e over an atom's partners (994-996), clash_atom = any flag (1006-1009), clash_atom_pairs =
//             the partners counted; clash_mean_loss = sum of e over unordered pairs / (1e-6 + pairs counted) (990) = half the
//             sum of clash_atom_loss over half the sum of clash_atom_pairs, in fp64, per sample.
//   group     the *_cross outputs keep only partners whose residue has another group byte.
//   query     only pairs with at least one atom in a query residue are evaluated and counted.
//   Bond      connection n = (n, n + 1) for every n < N - 1, fp64 from the fp32 coordinates, eps 1e-6 inside the square roots.
//             C-N length against 1.329 +- 0.014 (1.341 +- 0.016 when n + 1 is a proline: aa == pro), cos(CA-C-N) against -0.4473,
//             cos(C-N-CA) against -0.5203 +- 0.0353 (residue_constants.py:546-551); error = sqrt(1e-6 + (value - ideal)^2), loss =
//             relu(error - factor * stddev), violation error > factor * stddev.  The CA-C-N test uses the BOND-LENGTH stddev 0.014,
//             not the angle's 0.0311 (loss.py:807): the reference's behaviour, kept.  A term's mask: its atoms exist (atom_mask) and
//             residue_index[n + 1] - residue_index[n] == 1.  The three means are masked sums / (mask count + 1e-6) (786-788).
//             connection_loss[n] = half the summed loss of connection n - 1 plus half that of connection n, and like the reference's
//             per_residue_loss_sum (841-847) it is NOT masked: gaps and absent atoms contribute what their coordinates give.
//             connection_violation[n] = a masked violation on connection n - 1 or n (850-860).
//   CA-CA     ca_ca_break[n] = both CA exist, no gap, sqrt(1e-6 + |CA(n) - CA(n+1)|^2) - 3.80209737096 > 1.5 (1256-1268);
//             ca_ca_extreme = breaks / (1e-4 + connections tested) (tensor_utils.py:32-34).
//
// Two launches, no atomics, no scratch, nothing pair-sized: every output has one writer and every sum a fixed order, so the
// results are bit-identical from run to run and do not depend on the rest of the batch.
//   clash_kernel       grid (row tiles of 16 residues, B), 256 threads, thread t < 224 owns atom (t / 14, t % 14) of the row tile.
//                      Column tiles of 16 residues are staged in LDS as (x, y, z, radius) float4 (radius 0: no atom) plus index and
//                      flags per residue, double-buffered, the next tile fetched into registers while the current one is
//                      evaluated; all lanes read the same LDS word (broadcast).  The column tiles to visit come from a list
//                      built in LDS 256 tiles at a time: every tile, or with `query` and no query residue in the row tile only
//                      those that hold one.
//   reduce_kernel      one block per sample: the connection pass (a thread per residue) and the per-sample means.
#include "common.h"
#include "../../include/pepflow_hip.h"
#include "eval_dev.h"

namespace {

constexpr int TR = 16, SL = 14, TA = TR * SL;       // residues per tile, slots per residue, atoms per tile
constexpr int NT = 256;
constexpr unsigned char F_QUERY = 1, F_GROUP = 2, F_VALID = 4;

constexpr double CA_CA = 3.80209737096, CA_CA_TOL = 1.5;
constexpr double CN_LEN = 1.329, CN_LEN_PRO = 1.341, CN_SD = 0.014, CN_SD_PRO = 0.016;
constexpr double COS_CA_C_N = -0.4473, COS_C_N_CA = -0.5203, COS_C_N_CA_SD = 0.0353;
constexpr double BOND_EPS = 1e-6;

struct Tile {
    float4 at[TA];
    int idx[TR];
    unsigned char flg[TR];
};

struct Fetched {
    float4 at;
    int idx;
    unsigned char flg;
};

// thread t < 224: atom t of column tile ct; thread t < 16: residue t of it.  Loads come from clamped (valid) addresses.
__device__ __forceinline__ Fetched fetch_tile(const pf_violations_args& a, size_t b, int ct, int tid) {
    Fetched f;
    f.at = make_float4(0.f, 0.f, 0.f, 0.f);
    f.idx = 0;
    f.flg = 0;
    const int N = a.N;
    if (tid < TA) {
        const int q = ct * TR + tid / SL, s = tid % SL;
        const size_t r = b * N + (q < N ? q : N - 1);
        const float* p = a.pos + (r * a.n_atoms + s) * 3;
        const int64_t t = a.aa[r];
        const float rad = a.radius[(t < 0 || t > 20 ? 20 : (int)t) * SL + s];
        const bool ok = q < N && a.atom_mask[r * a.n_atoms + s] != 0;
        f.at = make_float4(p[0], p[1], p[2], ok ? rad : 0.f);
    }
    if (tid < TR) {
        const int q = ct * TR + tid;
        const size_t r = b * N + (q < N ? q : N - 1);
        f.idx = a.residue_index[r];
        f.flg = (unsigned char)((a.query && a.query[r] ? F_QUERY : 0) | (a.group && a.group[r] ? F_GROUP : 0) | (q < N ? F_VALID : 0));
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

__global__ __launch_bounds__(NT) void clash_kernel(pf_violations_args a) {
    __shared__ Tile tile[2];
    __shared__ int list[NT];
    __shared__ int wcnt[NT / 64];
    const int N = a.N, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.y;
    const int rt = blockIdx.x, n_tiles = (N + TR - 1) / TR;
    const float tol = a.clash_overlap_tolerance;
    const bool has_query = a.query != nullptr;

    // the thread's own atom
    const int p = rt * TR + tid / SL, s = tid % SL;
    const bool row = tid < TA && p < N;
    float4 own = make_float4(0.f, 0.f, 0.f, 0.f);
    int idx_p = 0;
    unsigned char flg_p = 0;
    if (row) {
        const size_t r = b * N + p;
        const float* q = a.pos + (r * a.n_atoms + s) * 3;
        const int64_t t = a.aa[r];
        const float rad = a.radius[(t < 0 || t > 20 ? 20 : (int)t) * SL + s];
        own = make_float4(q[0], q[1], q[2], a.atom_mask[r * a.n_atoms + s] ? rad : 0.f);
        idx_p = a.residue_index[r];
        flg_p = (unsigned char)((has_query && a.query[r] ? F_QUERY : 0) | (a.group && a.group[r] ? F_GROUP : 0));
    }
    const bool all_tiles = !has_query || __syncthreads_or(row && (flg_p & F_QUERY));

    float loss = 0.f, loss_x = 0.f;
    int pairs = 0;
    bool flag = false, flag_x = false;

    for (int chunk = 0; chunk < n_tiles; chunk += NT) {
        // the column tiles of this chunk that hold work, in ascending order
        const int ct = chunk + tid;
        bool work = ct < n_tiles;
        if (work && !all_tiles) {
            work = false;
            const unsigned char* qr = a.query + b * N;
            for (int r = ct * TR; r < min(N, ct * TR + TR); ++r) work = work || qr[r] != 0;
        }
        const unsigned long long bal = __ballot(work);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int off = __popcll(bal & ((1ull << lane) - 1ull)), cnt = 0;
        for (int w = 0; w < NT / 64; ++w) {
            if (w < wave) off += wcnt[w];
            cnt += wcnt[w];
        }
        if (work) list[off] = ct;
        __syncthreads();

        if (cnt > 0) {
            commit_tile(tile[0], fetch_tile(a, b, list[0], tid), tid);
            __syncthreads();
        }
        for (int k = 0; k < cnt; ++k) {
            Fetched next;
            const bool more = k + 1 < cnt;
            if (more) next = fetch_tile(a, b, list[k + 1], tid);
            const Tile& T = tile[k & 1];
            if (own.w > 0.f) {
                for (int r = 0; r < TR; ++r) {
                    const int idx_q = T.idx[r];
                    const unsigned char f = T.flg[r];
                    if (!(f & F_VALID) || idx_q == idx_p) continue;
                    if (has_query && !((f | flg_p) & F_QUERY)) continue;
                    const bool cross = ((f ^ flg_p) & F_GROUP) != 0;
                    const bool cn_next = s == 2 && (long long)idx_p + 1 == idx_q;      // own C, N of the next index
                    const bool cn_prev = s == 0 && (long long)idx_q + 1 == idx_p;      // own N, C of the previous index
#pragma unroll
                    for (int t = 0; t < SL; ++t) {
                        const float4 c = T.at[r * SL + t];
                        if (!(c.w > 0.f) || (t == 5 && s == 5) || (t == 0 && cn_next) || (t == 2 && cn_prev)) continue;
                        ++pairs;
                        const float lim = (own.w + c.w) - tol;
                        const float dx = own.x - c.x, dy = own.y - c.y, dz = own.z - c.z;
                        const float d2 = (dx * dx + dy * dy) + dz * dz;
                        if (lim > 0.f && d2 < lim * lim * 1.0001f) {                    // a superset of d < lim
                            const float d = sqrtf(1e-10f + d2);
                            if (d < lim) {
                                const float e = lim - d;
                                loss += e;
                                flag = true;
                                if (cross) {
                                    loss_x += e;
                                    flag_x = true;
                                }
                            }
                        }
                    }
                }
            }
            if (more) commit_tile(tile[(k + 1) & 1], next, tid);
            __syncthreads();
        }
    }

    if (row) {
        const size_t o = (b * N + p) * SL + s;
        a.clash_atom_loss[o] = loss;
        a.clash_atom[o] = flag;
        a.clash_atom_pairs[o] = pairs;
        if (a.clash_atom_loss_cross) {
            a.clash_atom_loss_cross[o] = loss_x;
            a.clash_atom_cross[o] = flag_x;
        }
    }
}

struct Conn {
    double loss;            // the three losses, unmasked
    double l_cn, l_a1, l_a2;
    bool m_cn, m_a1, m_a2, m_ca;
    bool viol, ca_break;
};

__device__ __forceinline__ double dist_eps(const double p[3], const double q[3]) {
    const double x = p[0] - q[0], y = p[1] - q[1], z = p[2] - q[2];
    return sqrt(BOND_EPS + ((x * x + y * y) + z * z));
}

// connection (n, n + 1) of sample b, 0 <= n < N - 1
__device__ __forceinline__ Conn connection(const pf_violations_args& a, size_t b, int n) {
    const size_t r0 = b * a.N + n, r1 = r0 + 1;
    const float* P0 = a.pos + r0 * a.n_atoms * 3;
    const float* P1 = a.pos + r1 * a.n_atoms * 3;
    const unsigned char* M0 = a.atom_mask + r0 * a.n_atoms;
    const unsigned char* M1 = a.atom_mask + r1 * a.n_atoms;
    double ca[3], c[3], n1[3], ca1[3];
    load3d(P0 + 3, ca);
    load3d(P0 + 6, c);
    load3d(P1, n1);
    load3d(P1 + 3, ca1);
    const bool nogap = (long long)a.residue_index[r1] - (long long)a.residue_index[r0] == 1;
    const bool pro = a.aa[r1] == a.pro;
    const double tf = (double)a.violation_tolerance_factor;

    Conn o;
    const double cn = dist_eps(c, n1), cac = dist_eps(ca, c), nca = dist_eps(n1, ca1);
    const double len = pro ? CN_LEN_PRO : CN_LEN, sd = pro ? CN_SD_PRO : CN_SD;
    const double e_cn = sqrt(BOND_EPS + (cn - len) * (cn - len));
    o.l_cn = fmax(e_cn - tf * sd, 0.0);
    o.m_cn = M0[2] && M1[0] && nogap;

    double u_cca[3], u_cn[3], u_nca[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u_cca[k] = (ca[k] - c[k]) / cac;
        u_cn[k] = (n1[k] - c[k]) / cn;
        u_nca[k] = (ca1[k] - n1[k]) / nca;
    }
    const double cos1 = (u_cca[0] * u_cn[0] + u_cca[1] * u_cn[1]) + u_cca[2] * u_cn[2];
    const double e_a1 = sqrt(BOND_EPS + (cos1 - COS_CA_C_N) * (cos1 - COS_CA_C_N));
    o.l_a1 = fmax(e_a1 - tf * CN_SD, 0.0);                          // the bond-length stddev: loss.py:807
    o.m_a1 = M0[1] && M0[2] && M1[0] && nogap;

    const double cos2 = ((-u_cn[0]) * u_nca[0] + (-u_cn[1]) * u_nca[1]) + (-u_cn[2]) * u_nca[2];
    const double e_a2 = sqrt(BOND_EPS + (cos2 - COS_C_N_CA) * (cos2 - COS_C_N_CA));
    o.l_a2 = fmax(e_a2 - tf * COS_C_N_CA_SD, 0.0);
    o.m_a2 = M0[2] && M1[0] && M1[1] && nogap;

    o.loss = (o.l_cn + o.l_a1) + o.l_a2;
    o.viol = (o.m_cn && e_cn > tf * sd) || (o.m_a1 && e_a1 > tf * CN_SD) || (o.m_a2 && e_a2 > tf * COS_C_N_CA_SD);
    o.m_ca = M0[1] && M1[1] && nogap;
    o.ca_break = o.m_ca && dist_eps(ca, ca1) - CA_CA > CA_CA_TOL;
    return o;
}

__global__ __launch_bounds__(NT) void reduce_kernel(pf_violations_args a) {
    __shared__ double red[NT];
    const int N = a.N, tid = threadIdx.x;
    const size_t b = blockIdx.x;

    double s_cn = 0.0, s_a1 = 0.0, s_a2 = 0.0, c_cn = 0.0, c_a1 = 0.0, c_a2 = 0.0, s_ca = 0.0, c_ca = 0.0;
    for (int n = tid; n < N; n += NT) {
        double lsum = 0.0;
        bool viol = false, brk = false;
        if (n > 0) {
            const Conn o = connection(a, b, n - 1);
            lsum += 0.5 * o.loss;
            viol = o.viol;
        }
        if (n + 1 < N) {
            const Conn o = connection(a, b, n);
            lsum += 0.5 * o.loss;
            viol = viol || o.viol;
            brk = o.ca_break;
            if (o.m_cn) { s_cn += o.l_cn; c_cn += 1.0; }
            if (o.m_a1) { s_a1 += o.l_a1; c_a1 += 1.0; }
            if (o.m_a2) { s_a2 += o.l_a2; c_a2 += 1.0; }
            if (o.m_ca) { s_ca += brk ? 1.0 : 0.0; c_ca += 1.0; }
        }
        a.connection_loss[b * N + n] = (float)lsum;
        a.connection_violation[b * N + n] = viol;
        a.ca_ca_break[b * N + n] = brk;
    }
    double s_cl = 0.0, c_cl = 0.0;
    const size_t na = (size_t)N * SL;
    for (size_t i = tid; i < na; i += NT) {
        s_cl += (double)a.clash_atom_loss[b * na + i];
        c_cl += (double)a.clash_atom_pairs[b * na + i];
    }
    s_cn = block_sum<NT>(s_cn, red, tid); c_cn = block_sum<NT>(c_cn, red, tid);
    s_a1 = block_sum<NT>(s_a1, red, tid); c_a1 = block_sum<NT>(c_a1, red, tid);
    s_a2 = block_sum<NT>(s_a2, red, tid); c_a2 = block_sum<NT>(c_a2, red, tid);
    s_ca = block_sum<NT>(s_ca, red, tid); c_ca = block_sum<NT>(c_ca, red, tid);
    s_cl = block_sum<NT>(s_cl, red, tid); c_cl = block_sum<NT>(c_cl, red, tid);
    if (tid == 0) {
        a.bond_c_n_loss_mean[b] = (float)(s_cn / (c_cn + BOND_EPS));
        a.angle_ca_c_n_loss_mean[b] = (float)(s_a1 / (c_a1 + BOND_EPS));
        a.angle_c_n_ca_loss_mean[b] = (float)(s_a2 / (c_a2 + BOND_EPS));
        a.ca_ca_extreme[b] = (float)(s_ca / (1e-4 + c_ca));
        a.clash_mean_loss[b] = (float)(0.5 * s_cl / (1e-6 + 0.5 * c_cl));
    }
}

}  // namespace

extern "C" int pf_violations_fwd(const pf_violations_args* a, pf_stream_t stream) {
    if (!a || !a->pos || !a->atom_mask || !a->aa || !a->residue_index || !a->radius || a->B < 0 || a->N < 0 || a->n_atoms < SL ||
        !a->clash_atom_loss || !a->clash_atom || !a->clash_atom_pairs || !a->clash_mean_loss || !a->bond_c_n_loss_mean ||
        !a->angle_ca_c_n_loss_mean || !a->angle_c_n_ca_loss_mean || !a->connection_loss || !a->connection_violation ||
        !a->ca_ca_break || !a->ca_ca_extreme || (!a->clash_atom_loss_cross != !a->clash_atom_cross) ||
        (a->clash_atom_loss_cross && !a->group))
        return PF_E_BADARG;
    if (a->B > 65535) return PF_E_TOOLARGE;
    if (a->B == 0) return 0;
    if (a->N > 0) {
        hipLaunchKernelGGL(clash_kernel, dim3((unsigned)((a->N + TR - 1) / TR), (unsigned)a->B), dim3(NT), 0, (hipStream_t)stream, *a);
        PF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)a->B), dim3(NT), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
