// pf_cluster_fwd -- the samples of each group clustered on a pairwise distance matrix: Daura's neighbour-count ("gromos") clustering
// (Daura et al., Angew. Chem. Int. Ed. 1999) and single / complete / average linkage cut at a height.  Written from the publications.
// The linkages are checked against scipy's fcluster(criterion="distance") as partitions only (tests/test_cluster_cpu.py, through the
// numpy restatement tests/cluster_oracle.py); gromos follows the publication and is not checked against GROMACS.
//
// Conventions (tests/cluster_oracle.py restates them in numpy):
//   Groups    index [B] lists the batch indices sorted by group, ascending inside a group; offsets [G+1] the groups' ranges in it.  A
//             sample's position is its rank inside its group.  d(a, b) for positions a < b is dist[index[a], index[b]]: the mirrored
//             entry and the diagonal are never read.  NaN counts as +inf and is never within a cutoff (a cutoff of +inf is taken as
//             FLT_MAX by the launcher).
//   gromos    neighbours of i: the j of the group with d(i, j) <= cutoff in fp32, i included.  Until no sample is active: the active
//             sample with the most active neighbours, of equal counts the smallest position, leaves with its active neighbours as the
//             next cluster.  Labels are the extraction order (sizes are then non-increasing); the representative is that centre.
//   linkage   from singletons, the pair of clusters (i < j, a cluster named by its smallest position) with the smallest linkage distance,
//             of equal distances the lexicographically smallest (i, j), merges while that distance is <= cutoff.  single: min,
//             complete: max, average: (n_i d_ik + n_j d_jk) / (n_i + n_j) in fp64 from the fp32 input, in this written order.  Labels:
//             by size descending, then by smallest position.  Representative: the medoid, the member with the smallest sum of
//             distances to the other members, each sum accumulated serially in fp64 in ascending position; of equal sums the smallest
//             position; a sum that holds +inf is +inf.
//   best      with score: the member of the own cluster with the lowest score, NaN last, of equal scores the smallest position.
//   n_neighbours   the gromos neighbour count over the whole group, for every method.
//
// One launch, one workgroup per group (256 threads up to n_max = 256, 1024 above), no atomics; every output has one writer and every
// choice is a minimum or maximum under a total order: the results are bit-identical from run to run and do not depend on the other groups.
//   neighbour bits   one wave per row reads the row's part right of the diagonal (and the diagonal word's lower part down its column),
//                    64 columns per ballot, every word of the row in flight at once; the words left of the diagonal word are then
//                    transposed out of LDS.  Rows are an odd number of 8-byte words apart, so 32 lanes reading one word of 32 rows fall
//                    into different bank pairs.  1024 x 17 words = 136 KiB at the bound.
//   gromos round     per active row popcount(row & active), packed with the position into one int, block maximum; when the best count
//                    is 1 everything left is a singleton and is labelled in one step.
//   linkage          the working matrix (symmetric, fp32; fp64 for average) lives in the caller's scratch; LDS keeps for each row its
//                    nearest active column to the right.  The global minimum over those is the pair to merge; a merge updates one row
//                    and one column and rescans (one wave per row) only the rows whose cached column was one of the two merged.
#include <float.h>
#include <limits.h>
#include <type_traits>
#include "common.h"
#include "../../include/pepflow_hip.h"

namespace {

typedef unsigned long long u64;
constexpr int MAXN = PF_CLUSTER_MAX_N, MAXW = MAXN / 64;
constexpr int SMALL_NT = 256, LARGE_NT = 1024;
constexpr int KEY_SHIFT = 11, KEY_POS = (1 << KEY_SHIFT) - 1;       // gromos key: count << 11 | (2047 - position)
static_assert(MAXN <= KEY_POS, "a position must fit the key");

// dynamic LDS: region A (the bit matrix; after it the linkage's row cache, the medoid sums, the scores), then five int arrays
__host__ __device__ inline int cl_stride(int n_max) { return ((n_max + 63) >> 6) | 1; }
__host__ __device__ inline size_t cl_region_a(int n_max) {
    const size_t bits = (size_t)n_max * cl_stride(n_max) * 8, link = (size_t)n_max * 24;
    return bits > link ? bits : link;
}
__host__ __device__ inline size_t cl_lds_bytes(int n_max) { return cl_region_a(n_max) + (size_t)n_max * 20; }

__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
    return v;
}

// (distance, index) total order: the smaller distance, of equal distances the smaller index
__device__ __forceinline__ bool pair_less(double d, int k, double d2, int k2) { return d < d2 || (d == d2 && k < k2); }

__device__ __forceinline__ void wave_argmin(double& d, int& k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double d2 = __shfl_xor(d, m);
        const int k2 = __shfl_xor(k, m);
        if (pair_less(d2, k2, d, k)) { d = d2; k = k2; }
    }
}

__device__ __forceinline__ float nan_to_inf(float v) { return v == v ? v : __builtin_inff(); }

// d(p, q) of two different positions from the caller's matrix: the entry right of the diagonal only
__device__ __forceinline__ float load_dist(const pf_cluster_args& a, const int* idx, int p, int q) {
    const int lo = p < q ? p : q, hi = p < q ? q : p;
    return a.dist[(size_t)idx[lo] * a.B + idx[hi]];
}

template <int NT, int METHOD>
__global__ __launch_bounds__(NT) void cluster_kernel(pf_cluster_args a, size_t work_stride, float cutoff) {
    constexpr int NW = NT / 64;
    constexpr bool LINK = METHOD != PF_CLUSTER_GROMOS;
    typedef typename std::conditional<METHOD == PF_CLUSTER_AVERAGE, double, float>::type T;
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ int red_i[NW];
    __shared__ double red_d[NW];
    __shared__ u64 active[MAXW], member[MAXW];
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = a.B, n_max = a.n_max;
    const int o0 = a.offsets[g], n = a.offsets[g + 1] - o0;
    if (o0 < 0 || n < 1 || n > n_max || n > B - o0) {                // uniform over the workgroup
        if (tid == 0) a.n_clusters[g] = 0;
        return;
    }
    const int stride = cl_stride(n_max), W = (n + 63) >> 6;
    u64* bits = reinterpret_cast<u64*>(smem);
    int* idx = reinterpret_cast<int*>(smem + cl_region_a(n_max));
    int *lab = idx + n_max, *csize = lab + n_max, *crep = csize + n_max, *cbest = crep + n_max;
    T* D = reinterpret_cast<T*>(static_cast<unsigned char*>(a.work) + (size_t)g * work_stride);      // LINK only

    int bad = 0;
    for (int p = tid; p < n; p += NT) {
        const int v = a.index[o0 + p];
        idx[p] = v;
        bad |= v < 0 || v >= B;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) a.n_clusters[g] = 0;
        return;
    }

    // ---- neighbour bits (and the working matrix): one wave per row, the whole row in flight
    for (int r = wave; r < n; r += NW) {
        const int w0 = r >> 6;
        float d[MAXW];
#pragma unroll
        for (int u = 0; u < MAXW; ++u) {
            const int c = 64 * u + lane;
            d[u] = __builtin_nanf("");
            if (u >= w0 && u < W && c < n && c != r) d[u] = load_dist(a, idx, r, c);
        }
#pragma unroll
        for (int u = 0; u < MAXW; ++u) {
            if (u >= w0 && u < W) {                                 // uniform over the wave
                const int c = 64 * u + lane;
                u64 bal = __ballot(d[u] <= cutoff);                 // NaN: never
                if (u == w0) bal |= 1ull << (r & 63);
                if (lane == 0) bits[(size_t)r * stride + u] = bal;
                if (LINK && c > r && c < n) {
                    const T v = (T)nan_to_inf(d[u]);
                    D[(size_t)r * n + c] = v;
                    D[(size_t)c * n + r] = v;
                }
            }
        }
    }
    __syncthreads();
    // the words left of the diagonal word: bit j of row r is bit r of row j, which lies right of row j's diagonal word
    for (int r = wave; r < n; r += NW) {
        const int w0 = r >> 6;
        for (int w = 0; w < w0; ++w) {
            const u64 bal = __ballot((bits[(size_t)(64 * w + lane) * stride + w0] >> (r & 63)) & 1ull);
            if (lane == 0) bits[(size_t)r * stride + w] = bal;
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
        int c = 0;
        for (int w = 0; w < W; ++w) c += __popcll(bits[(size_t)i * stride + w]);
        a.n_neighbours[idx[i]] = c;
    }

    int ncl = 0;
    if constexpr (!LINK) {
        if (tid < MAXW) active[tid] = tid >= W ? 0ull : (tid == W - 1 && (n & 63)) ? (1ull << (n & 63)) - 1ull : ~0ull;
        __syncthreads();
        int remaining = n;
        while (remaining > 0) {
            int key = -1;
            for (int i = tid; i < n; i += NT)
                if ((active[i >> 6] >> (i & 63)) & 1ull) {
                    int c = 0;
                    for (int w = 0; w < W; ++w) c += __popcll(bits[(size_t)i * stride + w] & active[w]);
                    key = max(key, (c << KEY_SHIFT) | (KEY_POS - i));
                }
            key = wave_max_int(key);
            if (lane == 0) red_i[wave] = key;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < NW; ++w) key = max(key, red_i[w]);
            const int c = key >> KEY_SHIFT, p = KEY_POS - (key & KEY_POS);
            if (c <= 1) {                                           // only singletons are left: in ascending position
                for (int i = tid; i < n; i += NT)
                    if ((active[i >> 6] >> (i & 63)) & 1ull) {
                        int below = __popcll(active[i >> 6] & ((1ull << (i & 63)) - 1ull));
                        for (int w = 0; w < (i >> 6); ++w) below += __popcll(active[w]);
                        lab[i] = ncl + below;
                        csize[i] = 1;
                        crep[i] = i;
                    }
                ncl += remaining;
                remaining = 0;
            } else {
                if (tid < W) member[tid] = bits[(size_t)p * stride + tid] & active[tid];
                __syncthreads();
                if (tid < W) active[tid] &= ~member[tid];
                for (int i = tid; i < n; i += NT)
                    if ((member[i >> 6] >> (i & 63)) & 1ull) {
                        lab[i] = ncl;
                        csize[i] = c;
                        crep[i] = p;
                    }
                ++ncl;
                remaining -= c;
                __syncthreads();
            }
        }
        __syncthreads();
    } else {
        // region A again: the nearest active column right of each row and its distance, cluster sizes, flags
        double* nd = reinterpret_cast<double*>(smem);
        int* nn = reinterpret_cast<int*>(smem + (size_t)8 * n_max);
        int* cnt = nn + n_max;
        unsigned char* alive = reinterpret_cast<unsigned char*>(cnt + n_max);
        unsigned char* need = alive + n_max;
        const double inf = __builtin_inf();
        __syncthreads();
        for (int i = tid; i < n; i += NT) {
            alive[i] = 1;
            need[i] = 1;
            cnt[i] = 1;
            lab[i] = i;
        }
        __syncthreads();
        ncl = n;
        for (;;) {
            for (int r = wave; r < n; r += NW) {
                if (!need[r]) continue;                             // uniform over the wave
                T v[MAXW];
#pragma unroll
                for (int u = 0; u < MAXW; ++u) {
                    const int c = 64 * u + lane;
                    v[u] = (T)inf;
                    if (u < W && c > r && c < n && alive[c]) v[u] = D[(size_t)r * n + c];
                }
                double bd = inf;
                int bm = INT_MAX;
#pragma unroll
                for (int u = 0; u < MAXW; ++u) {
                    const int c = 64 * u + lane;
                    if (u < W && c > r && c < n && alive[c] && (bm == INT_MAX || (double)v[u] < bd)) {
                        bd = (double)v[u];
                        bm = c;
                    }
                }
                wave_argmin(bd, bm);
                if (lane == 0) {
                    nd[r] = bd;
                    nn[r] = bm == INT_MAX ? -1 : bm;
                    need[r] = 0;
                }
            }
            __syncthreads();
            double bd = inf;
            int bi = INT_MAX;
            for (int i = tid; i < n; i += NT)
                if (alive[i] && nn[i] >= 0 && nd[i] < bd) {
                    bd = nd[i];
                    bi = i;
                }
            wave_argmin(bd, bi);
            if (lane == 0) {
                red_d[wave] = bd;
                red_i[wave] = bi;
            }
            __syncthreads();
            bd = red_d[0];
            bi = red_i[0];
#pragma unroll
            for (int w = 1; w < NW; ++w)
                if (pair_less(red_d[w], red_i[w], bd, bi)) { bd = red_d[w]; bi = red_i[w]; }
            if (bi == INT_MAX || !(bd <= (double)cutoff)) break;    // uniform over the workgroup
            const int i = bi, j = nn[i], ni = cnt[i], nj = cnt[j];
            __syncthreads();
            for (int k = tid; k < n; k += NT) {
                if (lab[k] == j) lab[k] = i;
                if (k == i || k == j || !alive[k]) continue;
                const T dik = D[(size_t)i * n + k], djk = D[(size_t)j * n + k];
                T nv;
                if constexpr (METHOD == PF_CLUSTER_SINGLE) nv = fminf(dik, djk);
                else if constexpr (METHOD == PF_CLUSTER_COMPLETE) nv = fmaxf(dik, djk);
                else nv = ((double)ni * dik + (double)nj * djk) / (double)(ni + nj);
                D[(size_t)i * n + k] = nv;
                D[(size_t)k * n + i] = nv;
                if (k < i) {
                    if (nn[k] == i || nn[k] == j) need[k] = 1;
                    else if (pair_less((double)nv, i, nd[k], nn[k])) { nd[k] = (double)nv; nn[k] = i; }
                } else if (k < j && nn[k] == j) need[k] = 1;
            }
            if (tid == 0) {
                alive[j] = 0;
                cnt[i] = ni + nj;
                need[i] = 1;
            }
            --ncl;
            __syncthreads();
        }
        // labels: by size descending, then by smallest position (the root)
        for (int r = tid; r < n; r += NT)
            if (alive[r]) {
                int rank = 0;
                for (int q = 0; q < n; ++q) rank += alive[q] && (cnt[q] > cnt[r] || (cnt[q] == cnt[r] && q < r));
                cbest[r] = rank;
            }
        __syncthreads();
        for (int p = tid; p < n; p += NT) {
            const int r = lab[p];
            lab[p] = cbest[r];
            csize[p] = cnt[r];
        }
        __syncthreads();
        // medoids: one thread per candidate, its sum serially in ascending position, from the caller's matrix
        double* dsum = nd;
        for (int p = tid; p < n; p += NT) {
            const int c = lab[p];
            double s = 0.0;
            if (csize[p] > 1)
                for (int q0 = 0; q0 < n; q0 += 8) {
                    float f[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int q = q0 + u;
                        f[u] = 0.f;
                        if (q < n && q != p && lab[q] == c) f[u] = load_dist(a, idx, p, q);
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int q = q0 + u;
                        if (q < n && q != p && lab[q] == c) s += (double)nan_to_inf(f[u]);
                    }
                }
            dsum[p] = s;
        }
        __syncthreads();
        for (int r = tid; r < n; r += NT)
            if (alive[r]) {
                const int c = lab[r];
                double bs = dsum[r];
                int bq = r;
                for (int q = r + 1; q < n; ++q)
                    if (lab[q] == c && dsum[q] < bs) {
                        bs = dsum[q];
                        bq = q;
                    }
                cnt[c] = bq;
            }
        __syncthreads();
        for (int p = tid; p < n; p += NT) crep[p] = cnt[lab[p]];
        __syncthreads();
    }

    if (a.score) {
        float* sc = reinterpret_cast<float*>(smem);
        for (int p = tid; p < n; p += NT) sc[p] = a.score[idx[p]];
        __syncthreads();
        for (int c = tid; c < ncl; c += NT) {
            float bs = 0.f;
            int bq = -1;
            for (int q = 0; q < n; ++q)
                if (lab[q] == c) {
                    const float s = sc[q];
                    if (bq < 0 || (s == s && (bs != bs || s < bs))) {
                        bs = s;
                        bq = q;
                    }
                }
            cbest[c] = bq;
        }
        __syncthreads();
    }
    for (int p = tid; p < n; p += NT) {
        const int o = idx[p];
        a.label[o] = lab[p];
        a.cluster_size[o] = csize[p];
        a.representative[o] = idx[crep[p]];
        if (a.score) a.best[o] = idx[cbest[lab[p]]];
    }
    if (tid == 0) a.n_clusters[g] = ncl;
}

template <int NT, int METHOD>
int launch(const pf_cluster_args& a, size_t work_stride, float cutoff, hipStream_t stream) {
    const size_t lds = cl_lds_bytes(a.n_max);
    // the raised limit is the dynamic part alone: with the kernel's static arrays it has to stay within the 160 KiB of a CU
    static PfOncePerDevice attr;
    if (lds > 64 * 1024 && attr.first()) {
        const hipError_t e = hipFuncSetAttribute((const void*)cluster_kernel<NT, METHOD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)cl_lds_bytes(MAXN));
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((cluster_kernel<NT, METHOD>), dim3((unsigned)a.G), dim3(NT), lds, stream, a, work_stride, cutoff);
    PF_CHECK_LAUNCH();
    return 0;
}

template <int METHOD>
int launch_method(const pf_cluster_args& a, size_t work_stride, float cutoff, hipStream_t stream) {
    return a.n_max <= SMALL_NT ? launch<SMALL_NT, METHOD>(a, work_stride, cutoff, stream)
                               : launch<LARGE_NT, METHOD>(a, work_stride, cutoff, stream);
}

}  // namespace

extern "C" int pf_cluster_work_bytes(int n_max, int method) {
    if (n_max < 1 || n_max > MAXN || method < PF_CLUSTER_GROMOS || method > PF_CLUSTER_AVERAGE) return -1;
    if (method == PF_CLUSTER_GROMOS) return 0;
    return n_max * n_max * (method == PF_CLUSTER_AVERAGE ? 8 : 4);
}

extern "C" int pf_cluster_fwd(const pf_cluster_args* a, pf_stream_t stream) {
    if (!a || !a->dist || !a->index || !a->offsets || !a->label || !a->cluster_size || !a->representative || !a->n_neighbours ||
        !a->n_clusters || a->B < 1 || a->G < 1 || a->n_max < 1 || a->method < PF_CLUSTER_GROMOS || a->method > PF_CLUSTER_AVERAGE ||
        !(a->cutoff >= 0.f) || (a->score && !a->best) || (a->method != PF_CLUSTER_GROMOS && !a->work))
        return PF_E_BADARG;
    if (a->n_max > MAXN) return PF_E_TOOLARGE;
    const float cutoff = a->cutoff < FLT_MAX ? a->cutoff : FLT_MAX;
    const size_t work_stride = (size_t)pf_cluster_work_bytes(a->n_max, a->method);
    hipStream_t s = (hipStream_t)stream;
    switch (a->method) {
        case PF_CLUSTER_GROMOS: return launch_method<PF_CLUSTER_GROMOS>(*a, work_stride, cutoff, s);
        case PF_CLUSTER_SINGLE: return launch_method<PF_CLUSTER_SINGLE>(*a, work_stride, cutoff, s);
        case PF_CLUSTER_COMPLETE: return launch_method<PF_CLUSTER_COMPLETE>(*a, work_stride, cutoff, s);
        default: return launch_method<PF_CLUSTER_AVERAGE>(*a, work_stride, cutoff, s);
    }
}
