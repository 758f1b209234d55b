// pf_cavity_fwd -- where on a receptor a peptide could bind: a LIGSITE-style buriedness scan (Hendlich, Rippmann & Barnickel, J. Mol.
// Graph. Model. 15, 1997) over a regular grid around a batch of heavy-atom structures, the connected cavities of the buried free
// points, their ranking and their lining residues.  The definitions are the contract; include/pepflow_hip.h lists them and
// tests/cavity_oracle.py restates them in numpy.
//
//   Grid      nx * ny * nz points, linear index i = (ix * ny + iy) * nz + iz (iz runs fastest), g = origin + (float)index * h per axis
//             in fp32 (a rounded product, a rounded sum).
//   Occupied  for some atom a with atom_mask set: ((dx*dx + dy*dy) + dz*dz) <= R_a*R_a, dx = gx - ax ..., R_a = radius[type, slot] +
//             probe, all fp32, no contraction.
//   Buried    of a free point: the number of the 7 lines through it (3 axes, then the diagonals (1,1,1), (1,1,-1), (1,-1,1),
//             (1,-1,-1)) with an occupied point within n_axis / n_diag steps in BOTH senses; a walk ends at the grid's edge.  255: occupied.
//   Cavities  components of the free points with buried >= min_buried under 6- or 26-connectivity; those of at least min_points
//             points, by size descending, ties by the smallest linear index of a member; the first max_cavities are reported.
//
// A fixed sequence of launches (and four memset nodes) on the caller's stream, nothing read back by the host:
//   occupy_kernel    a wave per residue, atom by atom: the points of the atom's conservative index box are tested over the lanes and
//                    the hits stored as bytes (1): idempotent, no atomics; atoms x (2R/h)^3 tests instead of points x atoms.
//   buried_kernel    a thread per point: the 14 walks (each ends at the first occupied point, at its step bound or at the edge) and the
//                    union-find's start: parent = the point's own index for a cavity point, -1 otherwise.
//   union_kernel     a thread per cavity point and its forward neighbours (3 or 13): roots are found through relaxed agent-scope atomic
//                    loads and linked with atomicMin, always the larger root under the smaller.  parent[x] <= x holds throughout, so
//                    there are no cycles, and a component's only root at the end is its smallest index whatever the order of the races.
//   flatten_kernel   parent = root for every cavity point, and the roots' sizes (integer atomicAdd).
//   collect_kernel   the roots of at least min_points points into a list (its order is arbitrary; nothing depends on it).
//   select_kernel    a block per structure: n_found, and max_cavities times the next component in the ranking's total order.
//   relabel_kernel   label = rank or -1; per cavity the members' index histograms along x, y, z and the sum of their buriedness
//                    (integer atomics: exact in any order).
//   finish_kernel    center = sum over an axis' histogram of count * (double)g in index order / size, rounded once; mean_buried.
//   lining_kernel    a wave per residue, as occupy_kernel with r_lining around each atom: a member point of cavity k within reach
//                    sets lining[k, residue] (byte stores of 1).
// Every loop has a bound that follows from the arguments: a walk n_axis / n_diag steps, an index box the grid, a path to a root and the
// retries of a link G = nx * ny * nz.  A loop that exhausts such a bound sets a bit of *status and ends; it never spins.
#include "common.h"
#include "../../include/pepflow_hip.h"
#include "eval_dev.h"

namespace {

constexpr int SL = PF_CAVITY_SLOTS, KMAX = PF_CAVITY_MAX_OUT;
constexpr int HEAD = 1 + 2 * KMAX;          // ints in front of the histograms: list length, selected roots, buriedness sums
constexpr int ST_PATH = 1, ST_LINK = 2, ST_LIST = 4;

struct Dims {
    int nx, ny, nz;
    size_t G;
    int small;                              // ints of a structure's zeroed head (HEAD + KMAX * (nx + ny + nz), rounded up to 4)
};

__host__ __device__ inline Dims dims_of(int nx, int ny, int nz) {
    Dims d;
    d.nx = nx, d.ny = ny, d.nz = nz;
    d.G = (size_t)nx * ny * nz;
    d.small = (HEAD + KMAX * (nx + ny + nz) + 3) & ~3;
    return d;
}

// work: [B][small + G] zeroed (head, sizes by root) | [B][G] parent | [B][G] list
struct Work {
    int *head, *csize, *parent, *list;
};
__device__ __forceinline__ Work work_of(const pf_cavity_args& a, const Dims& d, size_t b) {
    Work w;
    int* base = reinterpret_cast<int*>(a.work);
    const size_t zone = (size_t)d.small + d.G;
    w.head = base + b * zone;
    w.csize = w.head + d.small;
    w.parent = base + (size_t)a.B * zone + b * d.G;
    w.list = w.parent + (size_t)a.B * d.G;
    return w;
}

// the indices lo..hi of an axis that can lie within R of c: two indices of slack beyond the rounded quotient, clipped to the grid;
// a NaN coordinate gives an empty range
__device__ __forceinline__ void index_box(float c, float R, float o, float h, int n, int& lo, int& hi) {
    float fl = floorf(((c - R) - o) / h) - 2.f, fh = ceilf(((c + R) - o) / h) + 2.f;
    fl = fminf(fmaxf(fl, 0.f), (float)n);
    fh = fminf(fmaxf(fh, -1.f), (float)(n - 1));
    lo = (int)fl;
    hi = (int)fh;
}

__global__ __launch_bounds__(256) void occupy_kernel(pf_cavity_args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    const size_t b = blockIdx.y;
    if (r >= a.N) return;
    const Dims d = dims_of(a.nx, a.ny, a.nz);
    const size_t row = b * a.N + r;
    const int A = a.n_atoms, S = A < SL ? A : SL;
    const float* rad = a.radius + type_row(a.aa[row]) * SL;
    const float ox = a.origin[3 * b], oy = a.origin[3 * b + 1], oz = a.origin[3 * b + 2], h = a.h;
    unsigned char* occ = a.occupied + b * d.G;
    for (int s = 0; s < S; ++s) {
        if (!a.atom_mask[row * A + s]) continue;
        const float* p = a.pos + (row * A + s) * 3;
        const float ax = p[0], ay = p[1], az = p[2], R = rad[s] + a.probe, R2 = R * R;
        int x0, x1, y0, y1, z0, z1;
        index_box(ax, R, ox, h, d.nx, x0, x1);
        index_box(ay, R, oy, h, d.ny, y0, y1);
        index_box(az, R, oz, h, d.nz, z0, z1);
        const int wx = x1 - x0 + 1, wy = y1 - y0 + 1, wz = z1 - z0 + 1;
        if (wx <= 0 || wy <= 0 || wz <= 0) continue;
        const int n = wx * wy * wz;                         // <= G <= 2^21
        for (int t = lane; t < n; t += 64) {
            const int iz = z0 + t % wz, q = t / wz, iy = y0 + q % wy, ix = x0 + q / wy;
            const float gx = ox + (float)ix * h, gy = oy + (float)iy * h, gz = oz + (float)iz * h;
            const float dx = gx - ax, dy = gy - ay, dz = gz - az;
            if ((dx * dx + dy * dy) + dz * dz <= R2) occ[((size_t)ix * d.ny + iy) * d.nz + iz] = 1;
        }
    }
}

// an occupied point within n steps of (ix, iy, iz) along (sx, sy, sz); the walk ends at the grid's edge
__device__ __forceinline__ bool walk_hits(const unsigned char* occ, const Dims& d, int ix, int iy, int iz, int sx, int sy, int sz, int n) {
    for (int k = 1; k <= n; ++k) {
        ix += sx, iy += sy, iz += sz;
        if (ix < 0 || ix >= d.nx || iy < 0 || iy >= d.ny || iz < 0 || iz >= d.nz) return false;
        if (occ[((size_t)ix * d.ny + iy) * d.nz + iz]) return true;
    }
    return false;
}

__global__ __launch_bounds__(256) void buried_kernel(pf_cavity_args a) {
    const Dims d = dims_of(a.nx, a.ny, a.nz);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= d.G) return;
    const Work w = work_of(a, d, b);
    const unsigned char* occ = a.occupied + b * d.G;
    int v = 255;
    if (!occ[i]) {
        const int iz = (int)(i % d.nz), q = (int)(i / d.nz), iy = q % d.ny, ix = q / d.ny;
        constexpr int DIR[7][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};
        v = 0;
#pragma unroll
        for (int l = 0; l < 7; ++l) {
            const int n = l < 3 ? a.n_axis : a.n_diag;
            if (walk_hits(occ, d, ix, iy, iz, DIR[l][0], DIR[l][1], DIR[l][2], n) &&
                walk_hits(occ, d, ix, iy, iz, -DIR[l][0], -DIR[l][1], -DIR[l][2], n))
                ++v;
        }
    }
    a.buried[b * d.G + i] = (unsigned char)v;
    w.parent[i] = v != 255 && v >= a.min_buried ? (int)i : -1;
}

__device__ __forceinline__ int load_parent(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x: at most `bound` steps (every step goes to a smaller index); -1 and a status bit when the bound runs out
__device__ __forceinline__ int find_root(int* parent, int x, int bound, int* status) {
    for (int it = 0; it <= bound; ++it) {
        const int p = load_parent(parent + x);
        if (p == x) return x;
        if (p < 0 || p > x) break;                          // never for a cavity point: not followed
        x = p;
    }
    atomicOr(status, ST_PATH);
    return -1;
}

// the components of x and y become one: the larger root goes under the smaller; a root that another link took first is retried
__device__ __forceinline__ void unite(int* parent, int x, int y, int bound, int* status) {
    for (int it = 0; it <= bound; ++it) {
        x = find_root(parent, x, bound, status);
        y = find_root(parent, y, bound, status);
        if (x < 0 || y < 0 || x == y) return;
        if (x < y) {
            const int t = x;
            x = y, y = t;
        }
        const int old = atomicMin(parent + x, y);           // x > y
        if (old == x) return;
        x = old;                                            // x had a parent already: that one is united with y next
    }
    atomicOr(status, ST_LINK);
}

__global__ __launch_bounds__(256) void union_kernel(pf_cavity_args a) {
    const Dims d = dims_of(a.nx, a.ny, a.nz);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= d.G) return;
    const Work w = work_of(a, d, b);
    const unsigned char* bur = a.buried + b * d.G;
    const int mb = a.min_buried;
    if (bur[i] == 255 || bur[i] < mb) return;
    const int iz = (int)(i % d.nz), q = (int)(i / d.nz), iy = q % d.ny, ix = q / d.ny;
    // the neighbours after the point in (x, y, z) order: 3 of the 6, 13 of the 26
    constexpr int FWD[13][3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}, {0, 1, -1}, {0, 1, 1}, {1, -1, 0}, {1, 1, 0}, {1, 0, -1}, {1, 0, 1},
                                {1, -1, -1}, {1, -1, 1}, {1, 1, -1}, {1, 1, 1}};
    const int nf = a.connectivity == 26 ? 13 : 3;
    for (int f = 0; f < nf; ++f) {
        const int jx = ix + FWD[f][0], jy = iy + FWD[f][1], jz = iz + FWD[f][2];
        if (jx >= d.nx || jy < 0 || jy >= d.ny || jz < 0 || jz >= d.nz) continue;
        const size_t j = ((size_t)jx * d.ny + jy) * d.nz + jz;
        if (bur[j] == 255 || bur[j] < mb) continue;
        unite(w.parent, (int)i, (int)j, (int)d.G, a.status);
    }
}

__global__ __launch_bounds__(256) void flatten_kernel(pf_cavity_args a) {
    const Dims d = dims_of(a.nx, a.ny, a.nz);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= d.G) return;
    const Work w = work_of(a, d, b);
    if (load_parent(w.parent + i) < 0) return;
    // a parent that another thread flattens meanwhile is still an ancestor, and a root stays a root in this launch
    const int r = find_root(w.parent, (int)i, (int)d.G, a.status);
    if (r < 0) return;
    __hip_atomic_store(w.parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(w.csize + r, 1);
}

__global__ __launch_bounds__(256) void collect_kernel(pf_cavity_args a) {
    const Dims d = dims_of(a.nx, a.ny, a.nz);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= d.G) return;
    const Work w = work_of(a, d, b);
    if (w.parent[i] != (int)i || w.csize[i] < a.min_points) return;
    const int at = atomicAdd(w.head, 1);
    if ((size_t)at < d.G) w.list[at] = (int)i;
    else atomicOr(a.status, ST_LIST);
}

// (size, root) comes before (size2, root2) in the ranking
__device__ __forceinline__ bool ranks_before(int s, int r, int s2, int r2) { return s > s2 || (s == s2 && r < r2); }

__global__ __launch_bounds__(256) void select_kernel(pf_cavity_args a) {
    __shared__ int bs[256], br[256];
    const Dims d = dims_of(a.nx, a.ny, a.nz);
    const size_t b = blockIdx.x;
    const int tid = threadIdx.x, K = a.max_cavities;
    const Work w = work_of(a, d, b);
    int n = w.head[0];
    if ((size_t)n > d.G) n = (int)d.G;
    if (tid == 0) a.n_found[b] = n;
    int ps = 0x7fffffff, pr = -1;                           // the one chosen last: the next comes strictly after it
    for (int k = 0; k < K; ++k) {
        int s = -1, r = 0x7fffffff;
        for (int j = tid; j < n; j += 256) {
            const int rj = w.list[j], sj = w.csize[rj];
            if (ranks_before(ps, pr, sj, rj) && ranks_before(sj, rj, s, r)) s = sj, r = rj;
        }
        __syncthreads();
        bs[tid] = s, br[tid] = r;
        __syncthreads();
        for (int hlf = 128; hlf > 0; hlf >>= 1) {
            if (tid < hlf && ranks_before(bs[tid + hlf], br[tid + hlf], bs[tid], br[tid])) bs[tid] = bs[tid + hlf], br[tid] = br[tid + hlf];
            __syncthreads();
        }
        s = bs[0], r = br[0];
        if (tid == 0) {
            w.head[1 + k] = s < 0 ? -1 : r;
            a.size[b * K + k] = s < 0 ? 0 : s;
        }
        if (s >= 0) ps = s, pr = r;
        else ps = -1, pr = 0x7fffffff;                      // nothing is left: nothing comes after this either
    }
}

__global__ __launch_bounds__(256) void relabel_kernel(pf_cavity_args a) {
    __shared__ int sel[KMAX];
    const Dims d = dims_of(a.nx, a.ny, a.nz);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const Work w = work_of(a, d, b);
    const int K = a.max_cavities;
    if (threadIdx.x < KMAX) sel[threadIdx.x] = (int)threadIdx.x < K ? w.head[1 + threadIdx.x] : -1;
    __syncthreads();
    if (i >= d.G) return;
    const int p = w.parent[i];
    int lab = -1;
    if (p >= 0)
        for (int k = 0; k < K; ++k)
            if (sel[k] == p) lab = k;
    a.label[b * d.G + i] = lab;
    if (lab < 0) return;
    const int iz = (int)(i % d.nz), q = (int)(i / d.nz), iy = q % d.ny, ix = q / d.ny;
    int* hist = w.head + HEAD + (size_t)lab * (d.nx + d.ny + d.nz);
    atomicAdd(hist + ix, 1);
    atomicAdd(hist + d.nx + iy, 1);
    atomicAdd(hist + d.nx + d.ny + iz, 1);
    atomicAdd(w.head + 1 + KMAX + lab, (int)a.buried[b * d.G + i]);
}

__global__ __launch_bounds__(64) void finish_kernel(pf_cavity_args a) {
    const Dims d = dims_of(a.nx, a.ny, a.nz);
    const size_t b = blockIdx.x;
    const int k = threadIdx.x, K = a.max_cavities;
    if (k >= K) return;
    const Work w = work_of(a, d, b);
    const int size = a.size[b * K + k];
    float c[3] = {0.f, 0.f, 0.f}, mean = 0.f;
    if (size > 0) {
        const int* hist = w.head + HEAD + (size_t)k * (d.nx + d.ny + d.nz);
        const int len[3] = {d.nx, d.ny, d.nz};
        for (int ax = 0; ax < 3; ++ax) {
            const float o = a.origin[3 * b + ax];
            double sum = 0.0;
            for (int j = 0; j < len[ax]; ++j) sum += (double)hist[j] * (double)(o + (float)j * a.h);
            c[ax] = (float)(sum / (double)size);
            hist += len[ax];
        }
        mean = (float)((double)w.head[1 + KMAX + k] / (double)size);
    }
    for (int ax = 0; ax < 3; ++ax) a.center[(b * K + k) * 3 + ax] = c[ax];
    a.mean_buried[b * K + k] = mean;
}

__global__ __launch_bounds__(256) void lining_kernel(pf_cavity_args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;
    const size_t b = blockIdx.y;
    if (r >= a.N) return;
    const Dims d = dims_of(a.nx, a.ny, a.nz);
    const size_t row = b * a.N + r;
    const int A = a.n_atoms, S = A < SL ? A : SL, K = a.max_cavities;
    const float ox = a.origin[3 * b], oy = a.origin[3 * b + 1], oz = a.origin[3 * b + 2], h = a.h;
    const float R = a.r_lining, R2 = R * R;
    const int* label = a.label + b * d.G;
    unsigned hit = 0;
    for (int s = 0; s < S; ++s) {
        if (!a.atom_mask[row * A + s]) continue;
        const float* p = a.pos + (row * A + s) * 3;
        const float ax = p[0], ay = p[1], az = p[2];
        int x0, x1, y0, y1, z0, z1;
        index_box(ax, R, ox, h, d.nx, x0, x1);
        index_box(ay, R, oy, h, d.ny, y0, y1);
        index_box(az, R, oz, h, d.nz, z0, z1);
        const int wx = x1 - x0 + 1, wy = y1 - y0 + 1, wz = z1 - z0 + 1;
        if (wx <= 0 || wy <= 0 || wz <= 0) continue;
        const int n = wx * wy * wz;
        for (int t = lane; t < n; t += 64) {
            const int iz = z0 + t % wz, q = t / wz, iy = y0 + q % wy, ix = x0 + q / wy;
            const int lab = label[((size_t)ix * d.ny + iy) * d.nz + iz];
            if (lab < 0 || lab >= K) continue;
            const float gx = ox + (float)ix * h, gy = oy + (float)iy * h, gz = oz + (float)iz * h;
            const float dx = gx - ax, dy = gy - ay, dz = gz - az;
            if ((dx * dx + dy * dy) + dz * dz <= R2) hit |= 1u << lab;
        }
    }
    for (int k = 0; k < K; ++k)
        if (hit >> k & 1u) a.lining[(b * K + k) * a.N + r] = 1;
}

inline bool dims_ok(int nx, int ny, int nz) { return nx >= 1 && ny >= 1 && nz >= 1; }
inline bool dims_fit(int nx, int ny, int nz) {
    return (unsigned long long)nx * (unsigned long long)ny <= PF_CAVITY_MAX_POINTS &&
           (unsigned long long)nx * (unsigned long long)ny * (unsigned long long)nz <= PF_CAVITY_MAX_POINTS;
}

}  // namespace

extern "C" int pf_cavity_work_bytes(int nx, int ny, int nz) {
    if (!dims_ok(nx, ny, nz) || !dims_fit(nx, ny, nz)) return -1;
    const Dims d = dims_of(nx, ny, nz);
    return (int)(4 * ((size_t)d.small + 3 * d.G));
}

extern "C" int pf_cavity_fwd(const pf_cavity_args* a, pf_stream_t stream) {
    if (!a || !a->pos || !a->atom_mask || !a->aa || !a->radius || !a->origin || !a->work || !a->occupied || !a->buried || !a->label ||
        !a->n_found || !a->size || !a->center || !a->mean_buried || !a->lining || !a->status || a->B < 0 || a->N < 0 ||
        a->n_atoms < SL - 1 || !dims_ok(a->nx, a->ny, a->nz) || a->n_axis < 0 || a->n_diag < 0 || a->min_buried < 1 || a->min_buried > 7 ||
        (a->connectivity != 6 && a->connectivity != 26) || a->min_points < 1 || a->max_cavities < 1 || a->max_cavities > KMAX ||
        !(a->h > 0.f) || !(a->h < 1e6f) || !(a->probe >= 0.f) || !(a->probe < 1e6f) || !(a->r_lining >= 0.f) || !(a->r_lining < 1e6f))
        return PF_E_BADARG;
    if (a->N > PF_CAVITY_MAX_N || a->B > 65535 || !dims_fit(a->nx, a->ny, a->nz)) return PF_E_TOOLARGE;
    if (a->B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const Dims d = dims_of(a->nx, a->ny, a->nz);
    const size_t B = (size_t)a->B, K = (size_t)a->max_cavities;
    hipError_t e = hipMemsetAsync(a->work, 0, 4 * B * ((size_t)d.small + d.G), st);
    if (e == hipSuccess) e = hipMemsetAsync(a->occupied, 0, B * d.G, st);
    if (e == hipSuccess) e = hipMemsetAsync(a->status, 0, sizeof(int), st);
    if (e == hipSuccess && a->N > 0) e = hipMemsetAsync(a->lining, 0, B * K * (size_t)a->N, st);
    if (e != hipSuccess) return (int)e;
    const dim3 pts((unsigned)((d.G + 255) / 256), (unsigned)a->B), res((unsigned)((a->N + 3) / 4), (unsigned)a->B);
    if (a->N > 0) {
        hipLaunchKernelGGL(occupy_kernel, res, dim3(256), 0, st, *a);
        PF_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(buried_kernel, pts, dim3(256), 0, st, *a);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(union_kernel, pts, dim3(256), 0, st, *a);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(flatten_kernel, pts, dim3(256), 0, st, *a);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(collect_kernel, pts, dim3(256), 0, st, *a);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)a->B), dim3(256), 0, st, *a);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(relabel_kernel, pts, dim3(256), 0, st, *a);
    PF_CHECK_LAUNCH();
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)a->B), dim3(64), 0, st, *a);
    PF_CHECK_LAUNCH();
    if (a->N > 0) {
        hipLaunchKernelGGL(lining_kernel, res, dim3(256), 0, st, *a);
        PF_CHECK_LAUNCH();
    }
    return 0;
}
