// pf_seq_ratio_fwd, pf_seq_align_fwd, pf_seq_search_fwd -- sequence comparison of peptides of different lengths on the device: the
// difflib.SequenceMatcher ratio of the reference's `diff_ratio` (eval/geometry.py), Gotoh's affine-gap pairwise alignment (global and
// local) with a caller's substitution matrix, and the search of each query against a library of known sequences.  No substitution
// table is shipped, and there are no alignment statistics (E-values), profiles or multiple alignments.
//
// Conventions (tests/seq_oracle.py restates them in Python; the ratio is checked against difflib itself):
//   Sequences  pair p = (i, j) of pairs [P,2]: side x is the types aa_x[i] where mx[i] is set, in order, side y likewise from aa_y[j],
//              my[j].  A wave compacts a row in chunks of 64 residues (__ballot and a popcount prefix), so N, the padded length, is
//              not bounded here.  A type outside 0..19 becomes 20 ("X"); two X are equal.  Empty sequences are legal.  A compacted
//              length above PF_SEQ_MAX_LEN = 64 on either side, or a pair index out of range, writes the FILL VALUES; no address is
//              formed from the indices of such a pair.  "Compacted coordinates" below index the compacted sequences.
//   Ratio      Ratcliff-Obershelp as difflib.SequenceMatcher(None, a = x, b = y) does it.  There is no junk: autojunk only acts when
//              len(b) >= 200, which the 64 bound excludes.  The longest match of a window [alo,ahi) x [blo,bhi) is the longest common
//              substring inside it; of equal lengths the smallest start in a, then the smallest start in b.  A match (i, j, k), k > 0,
//              is recorded; the left window [alo,i) x [blo,j) and the right window [i+k,ahi) x [j+k,bhi) follow when both their sides
//              are non-empty.  matches = sum of k, total = len x + len y, ratio = 2.0 * matches / total in float64 (1.0 when total is
//              0): one IEEE division of the same integers as difflib's.  blocks [P,64,3]: the recorded (i, j, k) sorted by (i, j),
//              adjacent ones merged -- get_matching_blocks() without its sentinel -- unused rows (-1, -1, 0); n_blocks [P].
//              No recursion: a stack of 64 windows (the windows on it are disjoint and non-empty on both sides) and a `for` loop of
//              the constant trip bound 2 * 64 + 1 (a processed window either records a match, which uses up a letter of each side,
//              or records and pushes nothing).  Fill: ratio NaN, matches -1, total -1, n_blocks -1 (len_x, len_y: the lengths, -1 for
//              a bad index).
//   Alignment  Gotoh in int32.  matrix [21,21] int8, s = matrix[x_i][y_j]; a gap of length g costs gap_open + (g - 1) gap_extend,
//              0 <= gap_extend <= gap_open <= 4096.  With V = max(M, E, F):
//                E[i][j] = max(V[i][j-1] - gap_open, E[i][j-1] - gap_extend)      (a column of y against a gap)
//                F[i][j] = max(V[i-1][j] - gap_open, F[i-1][j] - gap_extend)      (a column of x against a gap)
//                V[i][j] = max(V[i-1][j-1] + s, F[i][j], E[i][j])
//              PF_SEQ_GLOBAL: end gaps are penalised, V[0][j] = E[0][j] = -gap_open - (j-1) gap_extend and its mirror; minus infinity
//              is INT_MIN / 2.  PF_SEQ_LOCAL: V = max(0, ...), the score is the largest cell, of equal cells the smallest i, then the
//              smallest j, and the alignment runs back until V is 0 (a score of 0: no columns, span 0 0 0 0).
//              Traceback ties: at V the diagonal first, then F, then E; inside E and F "opened here" before "extended".
//              Outputs [P]: score, n_ident (columns of equal types), n_aligned (columns without a gap), n_columns, the aligned span
//              [x_lo,x_hi) x [y_lo,y_hi) in compacted coordinates (the whole sequences in global mode), len_x, len_y, identity =
//              n_ident / n_columns in float64 (NaN without columns: the needle / water definition); x2y [P,64] (optional): the
//              y index aligned to the k-th residue of x, -1 for a gap or outside the span.  Fill: score INT_MIN, the counts and the
//              span -1, identity NaN, x2y -1.
//   Search     queries aa / mask [Q,N] against db_aa [D,Ld] (already compact, Ld <= 64) with db_len [D]: the library entry of the
//              highest alignment score, of equal scores the lowest index, with its n_ident, n_columns and identity.  An entry whose
//              db_len is outside [0, Ld] is never the best.  The Q x D scores are never stored.  A query above 64 residues, or no
//              valid entry (D = 0): best_index -1 and the alignment's fill values.
//
// No atomics, no scratch memory, one writer per output, integer arithmetic but for the one float64 division per pair: bit-identical
// from run to run, and a pair's result depends neither on the rest of the work list nor on its order.  Every loop has a constant
// trip bound or runs over a size argument (N / 64 chunks, D / 4 entries); none depends on the sequences' content.
//   seq_ratio_kernel   256 threads, one wave per pair.  Lane i owns letter i of x.  A window is swept column by column of y:
//                      run = equal ? (run of lane i-1 at the previous column) + 1 : 0 by __shfl_up, every lane keeps the largest key
//                      (run, 63 - start in x, 63 - start in y) and a wave maximum picks the match.  The window stack, the blocks and
//                      the two sequences live in LDS (wave-private: no workgroup barrier).
//   seq_align_kernel   256 threads, one wave per pair.  Lane i owns row i + 1; the anti-diagonal wavefront runs len x + len y - 1
//                      steps, the neighbour row's V and F come by __shfl_up, the row state stays in registers.  The traceback codes
//                      (one byte per cell: source of V, opened / extended of E and of F) go to 4 KiB of LDS per wave; the traceback
//                      is one serial walk of at most 128 steps that every lane follows (LDS broadcast reads).
//   seq_search_kernel  one workgroup of 4 waves per query; wave w aligns the entries w, w + 4, ... (score only, no traceback codes),
//                      keeps (score, lowest index), the four meet in LDS, and wave 0 aligns the winner once more with the traceback.
#include <limits.h>
#include <math.h>
#include "common.h"
#include "../../include/pepflow_hip.h"

namespace {

constexpr int ML = PF_SEQ_MAX_LEN, NTYPES = PF_SEQ_TYPES, NT = 256, WAVES = NT / 64;
constexpr int NEG = INT_MIN / 2;
static_assert(ML == 64, "one lane per residue of a wave");

// what a wave keeps in LDS; nothing of it is shared between waves
struct WaveLds {
    unsigned char xs[ML], ys[ML];       // the compacted types
    unsigned char tb[ML * ML];          // alignment: traceback codes, [row][column]; ratio: the first bytes hold the blocks
    int x2y[ML];                        // alignment: x2y; ratio: the window stack
    int out[3 * ML];                    // ratio: the merged blocks
};

// orders the LDS traffic of one wave: what a lane wrote before is what every lane reads after
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned char seq_type(long long v) { return (v < 0 || v > 19) ? (unsigned char)20 : (unsigned char)v; }

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, off);
        v = o > v ? o : v;
    }
    return v;
}

// the types of row `aa` where `m` is set, in order, into dst[0..63]; -> their count (what lies beyond 64 is counted, not stored)
__device__ __forceinline__ int seq_compact(const int64_t* __restrict__ aa, const unsigned char* __restrict__ m, int N,
                                           unsigned char* dst, int lane) {
    int n = 0;
    for (int c0 = 0; c0 < N; c0 += 64) {
        const int q = c0 + lane;
        const bool on = q < N && m[q] != 0;
        const unsigned long long b = __ballot(on);
        const int pos = n + __popcll(b & ((1ull << lane) - 1ull));
        if (on && pos < ML) dst[pos] = seq_type(aa[q]);
        n += __popcll(b);
    }
    return n;
}

__device__ __forceinline__ void load_matrix(signed char* mat, const signed char* __restrict__ src) {
    for (int t = threadIdx.x; t < NTYPES * NTYPES; t += NT) mat[t] = src[t];
    __syncthreads();
}

struct AlignRes {
    int score, n_ident, n_aligned, n_columns, x_lo, x_hi, y_lo, y_hi;
};

// One wave aligns w.xs[0..lx) with w.ys[0..ly), 0 <= lx, ly <= 64.  TB: with the traceback (fills w.tb and w.x2y); without it only
// `score` of the result is set.  Every lane returns the same values.
template <bool TB>
__device__ __forceinline__ AlignRes align_wave(WaveLds& w, const signed char* mat, int lx, int ly, bool local, int go, int ge, int lane) {
    AlignRes res;
    res.score = 0;
    res.n_ident = res.n_aligned = res.n_columns = 0;
    res.x_lo = res.y_lo = 0;
    res.x_hi = local ? 0 : lx;
    res.y_hi = local ? 0 : ly;
    if (TB) {
        w.x2y[lane] = -1;
        wave_sync();
    }
    if (lx == 0 || ly == 0) {                       // uniform: no cell
        const int g = lx + ly;                      // the length of the one gap
        if (!local && g > 0) {
            res.score = -go - (g - 1) * ge;
            res.n_columns = g;
        }
        return res;
    }

    // forward: lane i owns row r = i + 1; at step d it is at column c = d - i + 1
    const bool row_on = lane < lx;
    const int xi = row_on ? w.xs[lane] : 0;
    int Vl = local ? 0 : -go - lane * ge;                                   // V[r][c-1], starting from V[r][0]
    int El = NEG;                                                           // E[r][c-1], E[r][0]
    int dg = (local || lane == 0) ? 0 : -go - (lane - 1) * ge;              // V[r-1][c-1], starting from V[r-1][0]
    int Vc = NEG, Fc = NEG;                                                 // V, F of the own cell of the step before
    int best = 0, bestc = 1;
    const int nsteps = lx + ly - 1;
    for (int d = 0; d < 2 * ML - 1; ++d) {
        if (d >= nsteps) break;
        int upV = __shfl_up(Vc, 1), upF = __shfl_up(Fc, 1);                 // V[r-1][c], F[r-1][c]
        const int c = d - lane + 1;
        if (lane == 0) {
            upV = local ? 0 : -go - (c - 1) * ge;
            upF = NEG;
        }
        if (row_on && c >= 1 && c <= ly) {
            const int s = mat[xi * NTYPES + w.ys[c - 1]];
            const int eo = Vl - go, ee = El - ge, fo = upV - go, fe = upF - ge;
            const int E = ee > eo ? ee : eo, F = fe > fo ? fe : fo;
            int V = dg + s, src = 0;
            if (F > V) { V = F; src = 1; }
            if (E > V) { V = E; src = 2; }
            if (local && V <= 0) { V = 0; src = 3; }
            if (TB) w.tb[lane * ML + (c - 1)] = (unsigned char)(src | (ee > eo ? 4 : 0) | (fe > fo ? 8 : 0));
            if (V > best) { best = V; bestc = c; }
            dg = upV;
            Vl = V; El = E; Vc = V; Fc = F;
        }
    }

    int r, c;                                       // the cell the alignment ends in
    if (local) {
        // largest V; of equal ones the smallest row, then the smallest column (each lane kept its first).  V <= 127 * 64 < 2^13
        const unsigned key = wave_max_u32(best > 0 ? ((unsigned)best << 12) | ((unsigned)(63 - lane) << 6) | (unsigned)(ML - bestc) : 0u);
        if (key == 0) return res;
        res.score = (int)(key >> 12);
        r = 64 - (int)((key >> 6) & 63);
        c = ML - (int)(key & 63);
    } else {
        res.score = __shfl(Vc, lx - 1);
        r = lx;
        c = ly;
    }
    if (!TB) return res;
    res.x_hi = r;
    res.y_hi = c;

    // traceback: one walk, the same in every lane; each turn takes one column
    wave_sync();
    int state = 0;                                  // 0: in V, 1: in F, 2: in E
    for (int t = 0; t < 2 * ML; ++t) {
        if (r == 0 || c == 0) break;
        const int code = w.tb[(r - 1) * ML + (c - 1)];
        if (state == 0) {
            const int src = code & 3;
            if (src == 3) break;
            if (src == 0) {
                ++res.n_columns;
                ++res.n_aligned;
                res.n_ident += w.xs[r - 1] == w.ys[c - 1];
                if (lane == 0) w.x2y[r - 1] = c - 1;
                --r;
                --c;
                continue;
            }
            state = src;
        }
        ++res.n_columns;
        if (state == 1) {
            state = (code & 8) ? 1 : 0;
            --r;
        } else {
            state = (code & 4) ? 2 : 0;
            --c;
        }
    }
    if (local) {
        res.x_lo = r;
        res.y_lo = c;
    } else {
        res.n_columns += r + c;                     // the end gap that is left (one of the two is 0)
    }
    wave_sync();
    return res;
}

__device__ __forceinline__ double identity_of(const AlignRes& r) {
    return r.n_columns > 0 ? (double)r.n_ident / (double)r.n_columns : (double)NAN;
}

__global__ __launch_bounds__(NT) void seq_align_kernel(pf_seq_align_args a) {
    __shared__ WaveLds lds[WAVES];
    __shared__ signed char mat[NTYPES * NTYPES];
    load_matrix(mat, a.matrix);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * WAVES + wave;
    if (p >= a.P) return;                           // uniform over the wave; no workgroup barrier follows
    WaveLds& w = lds[wave];
    const int pi = a.pairs[2 * p], pj = a.pairs[2 * p + 1];
    const bool valid = pi >= 0 && pi < a.Bx && pj >= 0 && pj < a.By;
    int lx = -1, ly = -1;
    if (valid) {
        lx = seq_compact(a.aa_x + (size_t)pi * a.N, a.mx + (size_t)pi * a.N, a.N, w.xs, lane);
        ly = seq_compact(a.aa_y + (size_t)pj * a.N, a.my + (size_t)pj * a.N, a.N, w.ys, lane);
        wave_sync();
    }
    const bool ok = valid && lx <= ML && ly <= ML;
    AlignRes r;
    r.score = INT_MIN;
    r.n_ident = r.n_aligned = r.n_columns = r.x_lo = r.x_hi = r.y_lo = r.y_hi = -1;
    if (ok) r = align_wave<true>(w, mat, lx, ly, a.mode == PF_SEQ_LOCAL, a.gap_open, a.gap_extend, lane);
    if (a.x2y) a.x2y[(size_t)p * ML + lane] = ok ? w.x2y[lane] : -1;
    if (lane == 0) {
        a.score[p] = r.score;
        a.n_ident[p] = r.n_ident;
        a.n_aligned[p] = r.n_aligned;
        a.n_columns[p] = r.n_columns;
        a.x_lo[p] = r.x_lo;
        a.x_hi[p] = r.x_hi;
        a.y_lo[p] = r.y_lo;
        a.y_hi[p] = r.y_hi;
        a.len_x[p] = lx;
        a.len_y[p] = ly;
        a.identity[p] = ok ? identity_of(r) : (double)NAN;
    }
}

__device__ __forceinline__ unsigned pack_window(int alo, int ahi, int blo, int bhi) {
    return (unsigned)alo | ((unsigned)ahi << 7) | ((unsigned)blo << 14) | ((unsigned)bhi << 21);
}

__global__ __launch_bounds__(NT) void seq_ratio_kernel(pf_seq_ratio_args a) {
    __shared__ WaveLds lds[WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * WAVES + wave;
    if (p >= a.P) return;
    WaveLds& w = lds[wave];
    unsigned char* blk_j = w.tb;                    // the block that starts at letter i of x: its start in y and its length (0: none)
    unsigned char* blk_k = w.tb + ML;
    unsigned* stack = reinterpret_cast<unsigned*>(w.x2y);
    const int pi = a.pairs[2 * p], pj = a.pairs[2 * p + 1];
    const bool valid = pi >= 0 && pi < a.Bx && pj >= 0 && pj < a.By;
    int lx = -1, ly = -1;
    blk_k[lane] = 0;
    w.out[lane] = -1;
    w.out[ML + lane] = -1;
    w.out[2 * ML + lane] = -1;
    if (valid) {
        lx = seq_compact(a.aa_x + (size_t)pi * a.N, a.mx + (size_t)pi * a.N, a.N, w.xs, lane);
        ly = seq_compact(a.aa_y + (size_t)pj * a.N, a.my + (size_t)pj * a.N, a.N, w.ys, lane);
    }
    wave_sync();
    const bool ok = valid && lx <= ML && ly <= ML;
    int matches = -1, n_blocks = -1;
    if (ok) {
        const int xi = lane < lx ? w.xs[lane] : 255;
        int sp = 0;
        matches = 0;
        if (lx > 0 && ly > 0) {
            if (lane == 0) stack[0] = pack_window(0, lx, 0, ly);
            sp = 1;
        }
        for (int it = 0; it < 2 * ML + 1; ++it) {
            if (sp == 0) break;
            wave_sync();
            const unsigned win = stack[--sp];
            const int alo = win & 127, ahi = (win >> 7) & 127, blo = (win >> 14) & 127, bhi = (win >> 21) & 127;
            const bool in = lane >= alo && lane < ahi;
            int prev = 0;
            unsigned key = 0;
            for (int t = 0; t < ML; ++t) {
                const int j = blo + t;
                if (j >= bhi) break;
                int up = __shfl_up(prev, 1);
                if (lane == 0) up = 0;
                const int run = (in && xi == w.ys[j]) ? up + 1 : 0;
                if (run) {
                    const unsigned k = ((unsigned)run << 12) | ((unsigned)(63 - (lane - run + 1)) << 6) | (unsigned)(63 - (j - run + 1));
                    key = k > key ? k : key;
                }
                prev = run;
            }
            key = wave_max_u32(key);
            wave_sync();                            // the window has been read by every lane before its slot is written again
            if (key) {
                const int k = (int)(key >> 12), i = 63 - (int)((key >> 6) & 63), j = 63 - (int)(key & 63);
                matches += k;
                if (lane == 0) {
                    blk_j[i] = (unsigned char)j;
                    blk_k[i] = (unsigned char)k;
                }
                if (alo < i && blo < j && sp < ML) {
                    if (lane == 0) stack[sp] = pack_window(alo, i, blo, j);
                    ++sp;
                }
                if (i + k < ahi && j + k < bhi && sp < ML) {
                    if (lane == 0) stack[sp] = pack_window(i + k, ahi, j + k, bhi);
                    ++sp;
                }
            }
        }
        wave_sync();
        // the blocks in the order of their start in x (which is the order of their start in y), adjacent ones merged
        int i1 = 0, j1 = 0, k1 = 0;
        n_blocks = 0;
        for (int s = 0; s < ML; ++s) {
            const int k2 = blk_k[s];
            if (k2 == 0) continue;
            const int j2 = blk_j[s];
            if (i1 + k1 == s && j1 + k1 == j2) {
                k1 += k2;
            } else {
                if (k1) {
                    if (lane == 0) { w.out[3 * n_blocks] = i1; w.out[3 * n_blocks + 1] = j1; w.out[3 * n_blocks + 2] = k1; }
                    ++n_blocks;
                }
                i1 = s; j1 = j2; k1 = k2;
            }
        }
        if (k1) {
            if (lane == 0) { w.out[3 * n_blocks] = i1; w.out[3 * n_blocks + 1] = j1; w.out[3 * n_blocks + 2] = k1; }
            ++n_blocks;
        }
        wave_sync();
    }
    if (a.blocks) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int e = q * ML + lane;            // element e of the pair's [64,3] rows
            const int v = w.out[e];
            a.blocks[(size_t)p * 3 * ML + e] = (ok && e < 3 * n_blocks) ? v : (e % 3 == 2 ? 0 : -1);
        }
        if (lane == 0) a.n_blocks[p] = n_blocks;
    }
    if (lane == 0) {
        const int total = ok ? lx + ly : -1;
        a.matches[p] = matches;
        a.total[p] = total;
        a.len_x[p] = lx;
        a.len_y[p] = ly;
        a.ratio[p] = !ok ? (double)NAN : total > 0 ? 2.0 * (double)matches / (double)total : 1.0;
    }
}

__global__ __launch_bounds__(NT) void seq_search_kernel(pf_seq_search_args a) {
    __shared__ WaveLds lds[WAVES];
    __shared__ signed char mat[NTYPES * NTYPES];
    __shared__ int red_score[WAVES], red_index[WAVES];
    load_matrix(mat, a.matrix);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t q = blockIdx.x;
    WaveLds& w = lds[wave];
    const bool local = a.mode == PF_SEQ_LOCAL;
    // every wave compacts the query for itself: the same lx in all four
    const int lx = seq_compact(a.aa + q * a.N, a.mask + q * a.N, a.N, w.xs, lane);
    wave_sync();
    int best = INT_MIN, index = -1;
    if (lx <= ML) {
        for (int e = wave; e < a.D; e += WAVES) {   // ascending in each wave: `>` keeps the lowest index
            const int ly = a.db_len[e];
            if (ly < 0 || ly > a.Ld) continue;
            wave_sync();
            if (lane < ly) w.ys[lane] = seq_type(a.db_aa[(size_t)e * a.Ld + lane]);
            wave_sync();
            const int s = align_wave<false>(w, mat, lx, ly, local, a.gap_open, a.gap_extend, lane).score;
            if (index < 0 || s > best) { best = s; index = e; }
        }
    }
    if (lane == 0) {
        red_score[wave] = best;
        red_index[wave] = index;
    }
    __syncthreads();
    if (wave != 0) return;
    best = INT_MIN;
    index = -1;
#pragma unroll
    for (int v = 0; v < WAVES; ++v) {
        const int s = red_score[v], e = red_index[v];
        if (e >= 0 && (index < 0 || s > best || (s == best && e < index))) { best = s; index = e; }
    }
    AlignRes r;
    r.score = INT_MIN;
    r.n_ident = r.n_columns = -1;
    if (index >= 0) {
        const int ly = a.db_len[index];
        if (lane < ly) w.ys[lane] = seq_type(a.db_aa[(size_t)index * a.Ld + lane]);
        wave_sync();
        r = align_wave<true>(w, mat, lx, ly, local, a.gap_open, a.gap_extend, lane);
    }
    if (lane == 0) {
        a.best_index[q] = index;
        a.best_score[q] = r.score;
        a.best_n_ident[q] = r.n_ident;
        a.best_n_columns[q] = r.n_columns;
        a.best_identity[q] = index >= 0 ? identity_of(r) : (double)NAN;
    }
}

bool bad_scoring(const signed char* matrix, int mode, int gap_open, int gap_extend) {
    return !matrix || (mode != PF_SEQ_GLOBAL && mode != PF_SEQ_LOCAL) || gap_extend < 0 || gap_extend > gap_open || gap_open > PF_SEQ_MAX_GAP;
}

}  // namespace

extern "C" int pf_seq_ratio_fwd(const pf_seq_ratio_args* a, pf_stream_t stream) {
    if (!a || !a->aa_x || !a->aa_y || !a->mx || !a->my || !a->pairs || !a->ratio || !a->matches || !a->total || !a->len_x || !a->len_y ||
        (!a->blocks != !a->n_blocks) || a->Bx < 1 || a->By < 1 || a->N < 1 || a->P < 0)
        return PF_E_BADARG;
    if (a->P == 0) return 0;
    hipLaunchKernelGGL(seq_ratio_kernel, dim3((unsigned)((a->P + WAVES - 1) / WAVES)), dim3(NT), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}

extern "C" int pf_seq_align_fwd(const pf_seq_align_args* a, pf_stream_t stream) {
    if (!a || !a->aa_x || !a->aa_y || !a->mx || !a->my || !a->pairs || !a->score || !a->n_ident || !a->n_aligned || !a->n_columns ||
        !a->x_lo || !a->x_hi || !a->y_lo || !a->y_hi || !a->len_x || !a->len_y || !a->identity ||
        bad_scoring(a->matrix, a->mode, a->gap_open, a->gap_extend) || a->Bx < 1 || a->By < 1 || a->N < 1 || a->P < 0)
        return PF_E_BADARG;
    if (a->P == 0) return 0;
    hipLaunchKernelGGL(seq_align_kernel, dim3((unsigned)((a->P + WAVES - 1) / WAVES)), dim3(NT), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}

extern "C" int pf_seq_search_fwd(const pf_seq_search_args* a, pf_stream_t stream) {
    if (!a || !a->aa || !a->mask || !a->best_index || !a->best_score || !a->best_n_ident || !a->best_n_columns || !a->best_identity ||
        bad_scoring(a->matrix, a->mode, a->gap_open, a->gap_extend) || a->Q < 0 || a->N < 1 || a->D < 0 || a->Ld < 1 || a->Ld > ML ||
        (a->D > 0 && (!a->db_aa || !a->db_len)))
        return PF_E_BADARG;
    if (a->Q == 0) return 0;
    hipLaunchKernelGGL(seq_search_kernel, dim3((unsigned)a->Q), dim3(NT), 0, (hipStream_t)stream, *a);
    PF_CHECK_LAUNCH();
    return 0;
}
