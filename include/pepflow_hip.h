/*
 * pepflow_hip.h -- C ABI of libpepflow_hip.so: hand-written gfx950 (MI355X) kernels for the
 * PepFlow multi-modal flow-matching denoise path.
 *
 * The reference (Ced3-han/PepFlowww) has NO native/FFI interface for this path: it sits behind
 * a plain torch nn.Module API.  This header therefore DEFINES the boundary a
 * replacement must export; each entry point names the reference code it replaces
 * (paths relative to /root/reference).  The reference-side binding (ctypes) is shown in
 * INTEGRATION.md and implemented in pepflowww_amd/_capi.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch allocator); kernels never
 *     allocate, free or keep state; weights are read-only;
 *   - all float tensors are fp32, contiguous row-major unless a leading dimension (ld*) is given;
 *     sequences are int64; masks are fp32 0/1 ([B*L]);
 *   - launches go to the hipStream_t passed as `stream` (opaque void*), no device sync;
 *   - return value: hipError_t as int (0 = hipSuccess), PF_E_* (negative) for argument errors;
 *     nothing throws.
 */
#ifndef PEPFLOW_HIP_H
#define PEPFLOW_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_ABI_VERSION 65
#define PF_ATT_VROWS 164             /* rows of a head's transposed value block: 128 channels + 12 points x 3 */
/* att_vt (f16 mode, ABI 53): a head's transposed values [PF_ATT_VROWS rows][keys] in the FRAGMENT ORDER of the score kernel's second
 * product -- block (tile n, 32-key step) = 512 f16 = the eight operand slots of each of its 64 lanes: row c sits in tile n = c & 7 as
 * lane row r = c >> 3 (channels), or tile 8 + (c - 128) / 16 as r = (c - 128) % 16 (point coordinates); key j in step j / 32 at
 * K group (j / 8) % 4, slot j % 8.  PF_ATT_VT_HEAD(L) f16 per (sample, head); PF_ATT_VT_OFF(c, j, L) the offset of an element. */
#define PF_ATT_VT_NST(L) (((L) + 31) >> 5)
#define PF_ATT_VT_HEAD(L) ((size_t)11 * PF_ATT_VT_NST(L) * 512)
#define PF_ATT_VT_OFF(c, j, L) ((((size_t)(((c) < 128 ? ((c) & 7) : 8 + (((c) - 128) >> 4)) * PF_ATT_VT_NST(L) + ((j) >> 5)) * 64 + (((j) >> 3) & 3) * 16 + \
                                  ((c) < 128 ? ((c) >> 3) : (((c) - 128) & 15))) * 8) + ((j) & 7))
#define PF_E_BADARG (-1)
#define PF_E_TOOLARGE (-2)

typedef void* pf_stream_t;

/* model constants (configs/learn_angle.yaml:3-14) baked into the kernels */
#define PF_C_S 128
#define PF_C_Z 64
#define PF_HEADS 8
#define PF_C_HID 128
#define PF_QK_PTS 8
#define PF_V_PTS 12
#define PF_IPA_PROJ 3744  /* q 1024 | kv 2048 | q_pts 192 | kv_pts 480 */
#define PF_IPA_FEATS 1536 /* o 1024 | o_pt x,y,z 3*96 | |o_pt| 96 | o_pair 128 */
#define PF_ET_PRE 512     /* a 192 | c 192 | d 64 | e 64 */

int pf_abi_version(void);

/* MFMA fragment-layout self test: C[16,16] = A[16,K] * B[16,K]^T through the same tile
 * primitive every GEMM below uses.  K multiple of 16. */
int pf_selftest_mfma(const float* a, const float* b, float* c, int K, pf_stream_t stream);
/* Cross-lane primitive self test (DPP / permlane swaps used by every reduction): in[64] -> out[10][64] =
 * lane^1, lane^2, lane^4, lane^8 values; v+v[lane^16]; v+v[lane^32]; 16-lane row sum; wave sum; wave max; row max. */
int pf_selftest_lanes(const float* in, float* out, pf_stream_t stream);

/* ---- fused row-linear -------------------------------------------------------------------
 * y = epilogue(x W^T + bias), replaces torch.nn.Linear / ipa_pytorch.Linear (ipa_pytorch.py:116-181)
 * plus the element-wise ops the reference applies right after it:
 *   v = x W^T + bias ; relu ; v *= row_mask (mask_pre) ; v += residual ; LayerNorm(gamma,beta) ;
 *   v *= row_mask (mask_post)
 * covering ga.py:94-95,103-111, ipa_pytorch.py:196-206,478-482, TransformerEncoderLayer's
 * projections.  K must be a multiple of 16 (host pads); LayerNorm needs N <= 128. */
typedef struct {
    const float* x;  int ldx;
    const float* w;  int ldw;       /* [N, ldw], first K columns used */
    const float* bias;              /* [N] or NULL */
    float* y;        int ldy;
    int M, N, K;
    int relu;
    const float* row_mask;          /* [M] or NULL */
    int mask_pre, mask_post;
    const float* residual; int ldr; /* [M, ldr] or NULL */
    const float* ln_gamma; const float* ln_beta; float ln_eps; /* NULL = no LayerNorm */
    const void* w_f16;              /* optional: W pre-split into fragment-order f16 hi/lo planes (engine.split_f16);
                                       selects the split-precision MFMA path (bias / ReLU / row mask / gate / residual,
                                       K % 32 == 0, no LayerNorm) */
    const float* gate; int ldg;     /* split path only, optional: y = gate[m,n] > 0 ? y : 0 before the residual is added
                                       (backward of a ReLU fused into the dx product of the training path) */
    /* split path only, optional (IPA projection of the inference plan): output features n >= pt_col0 are point coordinates
     * packed (x, y, z, 0) per point -- 64 query points (h*8+p) then 160 key/value points (h*20+p; p < 8 key, else value) --
     * and are not stored to y: each point goes through the residue frame, R p + t (rigid_utils.py:1124-1150 via
     * ipa_pytorch.py:360-388), straight into qp [M,192] / kp [M,192] / vp [M,288] (what pf_ipa_points_fwd produces). */
    const float* pt_rot; const float* pt_trans; float* pt_qp; float* pt_kp; float* pt_vp; int pt_col0;
    int single_pass;                /* split path, 4-wave form only: 1 = f16 precision mode (one f16 MFMA per product, hi planes only) */
    /* split path with pt_* set (IPA projection of the inference plan), optional: write the attention operands as f16 planes
     * instead of fp32 `y` / `pt_vp` (csrc/ipa_split.hip consumes them; L = att_L must be a multiple of 16, M = B L):
     * single_pass only since ABI 50 (the hi / lo plane form of the fp32 mode was removed; att_qk without single_pass is refused):
     *   att_qk : M x 2048 f16 in all: the q rows [M][1024], then the k rows in the fragment order of the score kernel's first product
     *            (ABI 53) -- block (sample, head, 16-key tile, 32-channel K-step) = 512 f16 = the eight operand slots of each of the 64
     *            lanes: key tile row r, channel group kg = (c / 8) % 4 at lane kg * 16 + r, slot c % 8 (natural K order)
     *   att_vt : values TRANSPOSED per (sample, head), [B][8][PF_ATT_VT_HEAD(L)] f16 in the fragment order described at PF_ATT_VROWS
     *            (ABI 53; until then [PF_ATT_VROWS][L] rows: an operand load of the score kernel touched sixteen rows, 64 bytes of each) */
    void* att_qk; void* att_vt; int att_L;
    /* optional (split path): the rows are [B][key_L] residues and key_end[b] (device memory, int32 [B]) = 1 + the last unmasked
     * residue of sample b (the same list as pf_ipa_attn_args.key_end).  A row tile that lies entirely at or beyond its samples'
     * key ends is SKIPPED: x is not read, y / the point and attention outputs of those rows are NOT written (their consumers skip
     * the same rows; the caller keeps the buffers finite).  active_rows (host side hint, 0 = unknown) = sum of key_end: lets the
     * launcher pick the rows-persistent kernel when the ACTIVE tiles fit whole rounds of workgroups. */
    const int* key_end; int key_L; int active_rows;
    /* optional (split path with pt_* set, fp32 output, att_L = L a multiple of 16, M = B L; ABI 54): the k columns of the packed IPA
     * projection (features 1024 + 256 h .. + 127) go to k_frag INSTEAD of y, as fp32 fragments of the score kernel's first product:
     * block (sample, head, 16-key tile, 16-channel step) = 256 floats = the float4 of each of the 64 lanes (key r, channels 4 g ..);
     * M x 1024 floats in all.  pf_ipa_attn_args.k_frag takes the same buffer. */
    float* k_frag;
} pf_linear_args;
int pf_linear_fwd(const pf_linear_args* a, pf_stream_t stream);
/* W [N,K] fp32 (ldw) -- or W^T when `transpose` (then w is [K,N], ldw >= N) -- to the fragment-order f16 hi/lo planes
 * pf_linear_args.w_f16 expects ([2][ceil16(N)/16][K/32][64][8] f16, N zero-padded to 16): the device-side form of
 * engine.split_f16, used per step by the training path (weights change every step).  Layout only. */
int pf_split_pack_f16(const float* w, int ldw, int N, int K, int transpose, void* out, pf_stream_t stream);
/* the same for many matrices in ONE launch: desc (DEVICE memory, ndesc entries, ascending `first`) describes each matrix as above
 * (N rows of the packed matrix, K % 32 == 0) and the index of its first work item (= 8 consecutive k of one output row:
 * Npad * K / 8 items per matrix); total_items = the sum.  Same planes as pf_split_pack_f16, optional range flag as in *_checked. */
typedef struct { const float* w; int ldw, N, K, transpose; void* out; int first; int pad_; } pf_pack_desc;
int pf_split_pack_f16_batch(const pf_pack_desc* desc_dev, int ndesc, int total_items, int* range_flag, pf_stream_t stream);
/* the same, and *range_flag (device int, zeroed by the caller) is set to 1 if any |w| exceeds the f16 range (65504) or is not
 * finite: the split representation cannot carry such a weight (the packed value saturates); callers treat it as an error */
int pf_split_pack_f16_checked(const float* w, int ldw, int N, int K, int transpose, void* out, int* range_flag, pf_stream_t stream);

/* ---- input mixing features: ga.py:94 (cat) + ga.py:79-85 / utils.py:60-71 (time embedding) +
 * layers.py:92-113 (AngularEncoding, 12 funcs) + nn.Embedding lookup.
 * out[B*L, 640] = [node_embed 128 | seq_emb[seqs] 128 | time 128 | angle code 245 | 0 x 11] */
typedef struct {
    const float* node_embed;   /* [B*L,128] */
    const float* seq_table;    /* [22,128] */
    const int64_t* seqs;       /* [B*L] */
    const float* t;            /* [B] */
    const float* time_freq;    /* [64] host-computed exp(-k ln(2056)/63) */
    const float* ang_freq;     /* [24] AngularEncoding.freq_bands */
    const float* angles;       /* [B*L,5] */
    float* out;                /* [B*L,640] */
    int B, L;
} pf_embed_args;
int pf_embed_inputs_fwd(const pf_embed_args* a, pf_stream_t stream);
/* the same features, the two Linears of res_feat_mixer (ga.py:94-96: 640 -> 128 ReLU -> 128, masked) and the quaternion of
 * the current frames (rigid_utils.py:208-227) in ONE launch (csrc/node_track.hip: input_mixer_kernel); w0_f16 / w2_f16 are
 * the fragment-order f16 planes of mixer.0 (K padded 629 -> 640) and mixer.2 */
typedef struct {
    const float* node_embed; const float* seq_table; const int64_t* seqs; const float* t; const float* time_freq;
    const float* ang_freq; const float* angles;                       /* as in pf_embed_args */
    const void* w0_f16; const float* b0; const void* w2_f16; const float* b2;
    const float* mask;         /* [B*L] */
    const float* rot;          /* [B*L,9] current frames */
    float* quat;               /* [B*L,4] */
    float* s_out;              /* [B*L,128] */
    int B, L;
    int single_pass;           /* 1 = f16 precision mode: one f16 MFMA per product (hi weight planes only) */
    void* k_frag_s;            /* optional (appended, additive to ABI 65): the rows of s_out also as block 0's shared k fragments (pf_ipa_attn_args.k_frag_s) */
} pf_input_mixer_args;
int pf_input_mixer_fwd(const pf_input_mixer_args* a, pf_stream_t stream);

/* ---- rigid-body point projection: r.apply() on the IPA points, ipa_pytorch.py:360-387,
 * rigid_utils.py:1124 / 82-106.  proj row = [q|kv|q_pts|kv_pts]; outputs global-frame points. */
typedef struct {
    const float* proj; int ldp;    /* [B*L, ldp>=3744] */
    const float* rot;              /* [B*L,9] */
    const float* trans;            /* [B*L,3] */
    float* qp;                     /* [B*L, 8*8*3]  (h,p,xyz) */
    float* kp;                     /* [B*L, 8*8*3] */
    float* vp;                     /* [B*L, 8*12*3] */
    int rows;
} pf_ipa_points_args;
int pf_ipa_points_fwd(const pf_ipa_points_args* a, pf_stream_t stream);

/* ---- invariant point attention core: ipa_pytorch.py:389-475 (scores from scalar qk + pair bias +
 * point distances, masked softmax, o / o_pt / o_pair, inverse-frame projection, norms).
 * Reads z twice per query tile (bias pass, pair-value pass); never materialises the
 * [B,L,L,H,Pq,3] / [B,H,3,L,L,Pv] intermediates of the reference. */
typedef struct {
    const float* proj; int ldp;    /* [B*L, ldp] q at 0, kv at 1024 (per head: k 128 | v 128) */
    const float* qp; const float* kp; const float* vp; /* from pf_ipa_points_fwd */
    const float* z;                /* [B,L,L,64] */
    const float* rot; const float* trans; /* frames [B*L,9],[B*L,3] */
    const float* mask;             /* [B*L] */
    const float* w_b; const float* b_b;   /* linear_b  [8,64],[8]  */
    const float* w_dz; const float* b_dz; /* down_z    [16,64],[16] */
    const float* head_w;           /* [8] raw (softplus applied inside) */
    float* feats;                  /* [B*L,1536] */
    int B, L;
    /* optional: sqrt(1/3) (W_b z + b_b) precomputed per pair, [B,8,L,L] (head-major), by the producer of z
     * (pf_edge_transition_fwd bias_out, or pf_pair_bias_fwd): the bias pass over z is skipped, z is read once. */
    const float* bias;
    /* optional: the attention probabilities [B,8,L,L] are written here (the training backward keeps them).
     * With BOTH bias and p_out set and L <= 256 the two-kernel form runs (csrc/ipa_split.hip: scores per (sample, head),
     * then one streaming pass over z); otherwise the one-kernel form (csrc/ipa_attn.hip). */
    float* p_out;
    int variant;                   /* 0 = automatic; 1 = force the one-kernel form; 2 = demand the two-kernel form (error if impossible) */
    /* optional (two-kernel form, L % 16 == 0): the q / k / v operands as the f16 planes pf_linear_fwd (att_*) wrote; the score
     * kernel then runs its products on the f16 matrix instruction (single pass, att_mode = 2: the f16 mode) and `proj` / `vp` are
     * not read.  att_mode = 1 (hi / lo planes, 3-MFMA split) existed until ABI 50 as a test-only form and is refused now. */
    const void* att_qk; const void* att_vt; int att_mode;
    int head_group;                /* one-kernel form: 0 = head-group split by size; 2 / 4 / 8 = that variant */
    /* optional (two-kernel form): key_end[b] = 1 + the last unmasked residue of sample b (device memory, int32 [B]).  Keys and
     * query rows from key_end[b] on are skipped: their probabilities are exactly zero (mask term -1e5, ipa_pytorch.py:427-430) and
     * the outputs of masked query rows are multiplied by the mask afterwards (ga.py:104); feats / p_out there are NOT written. */
    const int* key_end;
    int z_f16;                     /* two-kernel form: z is [B,L,L,64] f16 (the f16 mode's pair tensor, see pf_edge_transition_args) */
    /* optional (two-kernel form): dz [B,L,L,16] fp32 = W_dz z without the bias (pf_edge_transition_args.dz_out, or pf_linear_fwd
     * of z for a pair tensor EdgeTransition did not produce): the pair aggregation sum_j P (W_dz z_j) + b_dz reads it instead of
     * z (which may then be NULL) */
    const float* dz;
    int dz_f16;                    /* dz is [B,L,L,16] f16 (the f16 mode: pf_edge_transition_args.dz_out_f16) */
    /* optional (two-kernel form with dz): 1 = the pair aggregation runs INSIDE the score kernel (the probabilities never leave the
     * workgroup: p_out is not written and may be NULL, no second kernel).  Needs fp32 dz with fp32 operands (proj) or f16 dz with
     * the f16 operand planes (att_*); other combinations fall back to the two-kernel form (which needs p_out). */
    int fused_pair;
    /* optional (two-kernel form, fp32 operands, L % 4 == 0, every query tile of a sample in one score workgroup: 64 <= L <= 128):
     * THE PROJECTION RUNS INSIDE THE SCORE KERNEL (ABI 50).  s_in [B*L,128] = the node state; proj_w_f16 = fragment-order hi / lo
     * planes (engine.split_f16) of the packed projection [3968,128] = [linear_q 1024 | linear_kv 2048 | 64 query points (x,y,z,0) |
     * 160 key / value points (x,y,z,0)] -- the matrix pf_linear_fwd takes with pt_col0 = 3072 -- and proj_bias [3968] its bias.
     * Each (sample, head) workgroup forms q and the query / key / value points (global frame, through rot / trans) on chip; `proj`
     * and qp / kp / vp are not touched in this form (proj must still be non-NULL).
     * fp32 operands (att_mode 0), ABI 51: `att_vt` is REQUIRED as the launch's SCRATCH of B x 8 x 512 x ceil32(L) f16 (1 KiB per key
     * and head; written through the const pointer): per (sample, head) the values as hi | lo f16 operand fragments of the second
     * product (transposed, fragment order: 1 KiB per (16-channel tile, 32-key step, plane)) and the k rows as operand fragments of
     * the first (8 KiB per 16-key tile: hi | lo f16 per 32-channel K-step without fused_pair, fp32 per 16-channel step with it) --
     * every operand load / store of the workgroup is one contiguous KiB.  The second product -- and without fused_pair the first --
     * runs as three f16 MFMAs per product (hi hi + hi lo + lo hi, ~2^-22 relative: the precision of every split-precision Linear of
     * this library) instead of fp32 MFMAs.  The buffer must hold FINITE values on entry (zero it
     * once): key columns at or beyond a sample's key end are not written and meet zero probabilities.
     * q, k and the points are bit-identical to pf_linear_fwd followed by the plain call; the outputs agree with it to ~1e-6 relative (ipa_pytorch.py:347-387 + 389-475 in one launch). */
    const float* s_in; const void* proj_w_f16; const float* proj_bias;
    /* optional (two-kernel form, fp32 operands without s_in, L % 16 == 0; ABI 54): the k rows as fp32 fragments written by pf_linear_fwd
     * (pf_linear_args.k_frag): the first product reads them instead of the k columns of `proj` -- one contiguous KiB per load instead of
     * sixteen rows x 64 bytes.  Same values, same arithmetic: results are bit-identical to the call without it. */
    const float* k_frag;
    /* optional (with s_in; ABI 58): 1 = THE KEYS ARE THE NODE STATE.  q_h . k_h = s_i^T (W_q,h^T W_k,h) s_j + terms constant along a softmax
     * row (ipa_pytorch.py:389-404,427-432), so when proj_w_f16 / proj_bias hold the query rows as W_k,h^T (W_q,h s + b_q,h)
     * (engine.fold_keys_into_queries: weights only) the k operand of the first product is the row of s_in itself: the kernel writes its
     * fragments from s_in and passes over the eight k tiles of the packed projection (whose rows are then never multiplied). */
    int k_from_s;
    /* optional (with k_from_s, fp32 operands, without fused_pair; appended, additive to ABI 65): the keys as hi | lo f16 operand fragments, ONE copy per sample
     * shared by its eight heads, [B][ceil(L / 16) tiles][8 KiB] f16: per 16-key tile and 32-channel K-step s 2 KiB (hi KiB, lo KiB), in
     * a KiB lane (key r, g) holds 16 bytes: halves 0..3 = channels 32 s + 4 g .. + 3, halves 4..7 = channels 32 s + 16 + 4 g .. + 3;
     * hi = f16(v), lo = f16(v - hi), unscaled.  Written by the producer of s_in (pf_input_mixer_args.k_frag_s / pf_node_tfmr_args.k_frag_s);
     * rows at or beyond a sample's key end only have to be finite.  NULL: the launch forms them itself (one small kernel in front,
     * into att_vt); the results are the same bytes either way.  Ignored by every other form. */
    const void* k_frag_s;
} pf_ipa_attn_args;
int pf_ipa_attn_fwd(const pf_ipa_attn_args* a, pf_stream_t stream);
/* 1 when pf_ipa_attn_fwd would run the projection-inside form (s_in) at this length (fp32 operands: f16_mode = 0; f16 operand
 * planes formed in LDS, att_mode 2: f16_mode = 1), 0 when it would refuse it (more than one score workgroup per (sample, head),
 * L % 4 / L % 16, LDS beyond 160 KiB): asked once per launch plan (ABI 55). */
int pf_ipa_proj_inside_ok(int L, int f16_mode);
/* the `bias` operand above for a pair tensor that EdgeTransition did not produce (block 0: edge_embed is constant over the
 * sampler steps -> computed once per sample() call): bias [B,8,L,L] = sqrt(1/3)(linear_b(z)), ipa_pytorch.py:393-404 */
int pf_pair_bias_fwd(const float* z, const float* w_b, const float* b_b, float* bias, int B, int L, pf_stream_t stream);

/* ---- sequence-transformer attention core (torch.nn.MultiheadAttention inside
 * nn.TransformerEncoderLayer, ga.py:53-62): 4 heads x 32, key padding mask. */
typedef struct {
    const float* qkv;              /* [B*L,384] q|k|v */
    const float* mask;             /* [B*L] */
    float* out;                    /* [B*L,128] */
    int B, L;
} pf_seq_attn_args;
int pf_seq_attn_fwd(const pf_seq_attn_args* a, pf_stream_t stream);

/* ---- fused node track of one GAEncoder block (csrc/node_track.hip) ----------------------------------
 * pf_node_head_fwd: s_ipa = LayerNorm(s + mask * linear_out(feats)) (ga.py:103-104, ipa_pytorch.py:478-482)
 *                   and qkv = in_proj(s_ipa) of seq_tfmr layer 0.  s_ipa may alias s_in. */
typedef struct {
    const float* feats;            /* [rows,1536] */
    const float* s_in;             /* [rows,128] */
    const float* mask;             /* [rows] */
    const void* w_out_f16; const float* b_out; /* ipa linear_out [128,1536], split planes */
    const float* ln_g; const float* ln_b;     /* ipa_ln */
    const void* w_in_f16; const float* b_in;   /* seq_tfmr layers.0.self_attn.in_proj [384,128], split planes */
    float* s_ipa;                  /* [rows,128] */
    float* qkv;                    /* [rows,384] */
    int rows;
    int single_pass;               /* 1 = f16 precision mode: one f16 MFMA per product (hi weight planes only) */
    /* optional: rows = [B][key_L]; row tiles entirely at or beyond their samples' key_end[b] are skipped (see pf_linear_args) */
    const int* key_end; int key_L;
    /* optional (training forward, fp32-parity mode): a0 = s_in + mask * linear_out(feats), the LayerNorm's input, [rows,128] */
    float* dump_a0;
    /* optional (ABI 57): 1 = the first 1024 columns of feats hold, per head h, that head's CONTRIBUTION to linear_out's output
     * (feats[:, 128 h + n] = sum_j P_h (W_out[:, 128 h : 128 h + 128] v_j)[n]: the value projection was multiplied by linear_out's
     * o-block when the weights were packed -- linear_out is linear and the softmax rows sum to one, ipa_pytorch.py:456,475-476).
     * The kernel then ADDS the eight head blocks (fixed order: ((h0 + h2) + h4) + h6, ((h1 + h3) + h5) + h7, the two sums) instead
     * of contracting them, and w_out_f16 is the [128, 512] matrix of the remaining columns (o_pt | o_pt_norm | o_pair): a third of
     * the weight stream and of the matrix work of this kernel.  Not with dump_a0. */
    int o_premul;
} pf_node_head_args;
int pf_node_head_fwd(const pf_node_head_args* a, pf_stream_t stream);

/* pf_node_tfmr_fwd: one post-LN nn.TransformerEncoderLayer (ga.py:53-62,105-106; d=128, 4 heads, ffn 128,
 * key padding mask) for 16 query rows per workgroup, followed by
 *   last == 0: the next layer's in_proj (qkv_out must not alias qkv: other workgroups still read K/V);
 *   last == 1: the block tail -- post_tfmr + residual (ga.py:107), StructureModuleTransition + mask
 *              (ga.py:108-109), BackboneUpdate + Rigid.compose_q_update_vec (ga.py:110-113) and, if has_et,
 *              EdgeTransition.initial_embed + its per-residue terms pre[rows,512] (ipa_pytorch.py:234-243).
 * s_out may alias s_ipa; quat/rot/trans may be updated in place. */
typedef struct {
    const float* qkv;              /* [B*L,384] this layer's q|k|v */
    const float* resid;            /* [B*L,128] layer input */
    const float* mask;             /* [B*L] */
    /* every *_f16 weight is the reference matrix [N,K] pre-split into fragment-order f16 planes (engine.split_f16) */
    const void* w_o_f16; const float* b_o; const float* n1_g; const float* n1_b;
    const void* w_1_f16; const float* b_1; const void* w_2_f16; const float* b_2; const float* n2_g; const float* n2_b;
    const void* w_in_next_f16; const float* b_in_next; float* qkv_out; float* v_out;   /* last == 0 */
    int last;
    const float* s_ipa;                                                                /* last == 1 ... */
    const void* w_post_f16; const float* b_post;
    const void* w_t1_f16; const float* b_t1; const void* w_t2_f16; const float* b_t2; const void* w_t3_f16; const float* b_t3;
    const float* nt_g; const float* nt_b;
    const void* w_bb_f16; const float* b_bb;   /* b_bb: bb_update bias [6] zero-padded to 8 floats */
    float* s_out;
    const float* quat_in; const float* rot_in; const float* trans_in;
    float* quat_out; float* rot_out; float* trans_out;
    int has_et;
    const void* w_init_f16; const float* b_init; const void* w_pre_f16; const float* b_pre; float* pre;
    int B, L;
    /* optional (last == 1, has_et == 0, i.e. the final block): the two output heads ga.py:123-124 on the new node
     * state while it is in LDS -- seq_net / angle_net = Linear(128,128)+ReLU, Linear(128,128)+ReLU, Linear(128,20|5);
     * h_w[net][layer] are fragment-order f16 planes (last layers padded to 32 / 16 rows), h_b[net][layer] the biases. */
    const void* h_w[2][3]; const float* h_b[2][3];
    float* logits_out;             /* [B*L,20] */
    float* ang_out;                /* [B*L,5] (before the % 2pi of ga.py:125) */
    int single_pass;               /* 1 = f16 precision mode: one f16 MFMA per product (hi weight planes only); the attention core,
                                      LayerNorms, residuals and the frame update stay fp32 */
    /* optional: query-row tiles that start at or beyond key_end[b] of their sample are skipped -- nothing of theirs is written
     * (s_out, frames, pre, qkv_out, v_out, logits_out, ang_out keep what they held; see pf_linear_args.key_end) */
    const int* key_end;
    /* optional (training forward; fp32-parity mode, <= 256 row tiles of 16): dump[k] != NULL for k < 5 (last == 0) / k < 11
     * (last == 1) -> the intermediates the backward needs are also stored, fp32 [B*L,128] each:
     *   0 att (attention output before out_proj)   1 h = out_proj(att) + x   2 x1 = LN1(h)   3 f = relu(linear1(x1))
     *   4 h2 = linear2(f) + x1      (the layer output LN2(h2) is v_out for last == 0, dump 5 for last == 1)
     *   5 tf = LN2(h2)   6 s2 = s_ipa + post_tfmr(tf)   7 t1   8 t2 (StructureModuleTransition hidden)   9 h3 = linear_3(t2) + s2
     *   10 the backbone update [B*L,8] (6 used: BackboneUpdate output, input of compose_q_update_vec) */
    float* dump[11];
    /* optional (last == 1, L % 16 == 0): row_on[(b L + i) / 16] != 0 marks the 16-row groups whose outputs are wanted; a query tile
     * without a marked group is skipped (nothing of it is written).  The sampler marks the groups that hold a generated residue in
     * the LAST block of a step: the predictions of context residues are replaced by the context anyway (flow_model.py:291-311). */
    const int* row_on;
    /* optional (last == 1; appended, additive to ABI 65; ignored by the training forward, i.e. with dump): the rows of s_out also as the next attention's shared
     * k fragments (pf_ipa_attn_args.k_frag_s, [B][ceil(L / 16)][8 KiB] f16), from the registers that hold them; skipped tiles keep what
     * they held */
    void* k_frag_s;
} pf_node_tfmr_args;
int pf_node_tfmr_fwd(const pf_node_tfmr_args* a, pf_stream_t stream);

/* ---- rot -> quat: rigid_utils.py:208-227 (top eigenvector of the 4x4 K matrix; the reference
 * calls torch.linalg.eigh, here a shifted power iteration converged to fp32). */
int pf_rot_to_quat(const float* rot, float* quat, int n, pf_stream_t stream);

/* ---- backbone update: Rigid.compose_q_update_vec, rigid_utils.py:1039-1063,587-616,266-275,
 * 331-332 and quat_to_rot 185-205.  In-place allowed. */
typedef struct {
    const float* quat_in;          /* [n,4] */
    const float* rot_in;           /* [n,9] rotation applied to the translation update */
    const float* trans_in;         /* [n,3] */
    const float* upd; int ldu;     /* [n,ldu>=6] */
    const float* mask;             /* [n] */
    float* quat_out; float* rot_out; float* trans_out;
    int n;
} pf_rigid_update_args;
int pf_rigid_update_fwd(const pf_rigid_update_args* a, pf_stream_t stream);

/* ---- EdgeTransition: ipa_pytorch.py:233-248 + edge mask ga.py:118.  The 192-wide concat
 * [z, n_i, n_j] is never built: pre[B*L,512] holds the per-residue terms
 *   a = W1[:,64:128] n, c = W1[:,128:192] n + b1, d = Wf[:,64:128] n, e = Wf[:,128:192] n + bf
 * (pf_node_tfmr_fwd tail, or pf_linear_fwd) and only the z part goes through the per-pair GEMMs.
 * Weights are passed PRE-SPLIT for the split-precision MFMA path: each *_f16 buffer holds the matrix as two
 * f16 planes (hi = f16(w), lo = f16((w - hi) * 2048)) in MFMA fragment order
 * [plane][N/16][K/32][64 lanes][8] -- produced by pepflowww_amd.engine.split_f16 (see csrc/common.h). */
typedef struct {
    const float* z_in;             /* [B*L*L,64] */
    float* z_out;                  /* may alias z_in; NULL (ABI 50, with bias_out set): z' is not stored -- the last EdgeTransition of a
                                    * step, whose output only feeds the next attention's pair bias / pair values (ga.py:115-118) */
    const float* pre;              /* [B*L,512] */
    const void* w1z_f16;           /* UNUSED since ABI 50 (operands of the round-1 tiled kernel, removed): leave NULL */
    const void* w2_f16;            /* UNUSED since ABI 50 */
    const float* b2;               /* trunk.2.bias [192] */
    const void* wf_f16;            /* UNUSED since ABI 50 */
    const float* ln_g; const float* ln_b;
    const float* mask;             /* [B*L] */
    int B, L;
    /* REQUIRED (this or w_stream32): trunk.0.weight[:, :64], trunk.2.weight and final_layer.weight as ONE 256 KiB stream of
     * 128 fragment pairs in consumption order (pepflowww_amd.engine.pack_et_stream) for the persistent LDS-ring kernel
     * (csrc/edge_transition_v3.hip).  The lo halves of the stream (and of
     * wb_frags) are f16(w - hi) UNSCALED -- this kernel adds all three products into one accumulator -- unlike the
     * w - hi times 2048 of every other split-precision operand (pf_split_pack_f16). */
    const void* w_stream;
    /* optional (persistent kernel only): also emit the NEXT block's IPA pair bias sqrt(1/3)(W_b z' + b_b)
     * from the normalised, masked z' while it is still in registers: bias_out [B,8,L,L] (head-major), wb_frags = linear_b
     * of the next block as 2 split-precision fragment pairs (pepflowww_amd.engine.pack_bias_frags), bb = its bias [8]. */
    float* bias_out; const void* wb_frags; const float* bb;
    /* optional (persistent kernel only; all three or none): the training forward keeps what the backward needs --
     * dump_h1 / dump_h2 [B*L*L,192] = relu(W1 x + b1), relu(W2 h1 + b2); dump_y [B*L*L,64] = the pre-LayerNorm output */
    float* dump_h1; float* dump_h2; float* dump_y;
    /* persistent kernel only: 1 = f16 precision mode -- ONE f16 MFMA per product (hi planes only) instead of the three of the
     * fp32-parity mode; fp32 accumulation, LayerNorm and storage unchanged.  Not combinable with the dumps. */
    int single_pass;
    /* optional (persistent kernel only): work list of the tiles that contain at least one unmasked pair.  A tile covers
     * pf_edge_transition_tile_rows(single_pass) rows i x 16 columns j of one sample; tile id = (b * nib + ib) * njb + jb with
     * nib = ceil(L / rows), njb = ceil(L / 16).  tile_list[0 .. *n_tiles) are processed, the others are NOT TOUCHED: z' of a fully
     * masked tile is exactly zero in the reference (ga.py:118), so the caller keeps those parts of z_out (and bias_out) zeroed.
     * Both pointers are device memory (the count is read by the kernel: no host synchronisation, graph-safe). */
    const int* tile_list; const int* n_tiles;
    /* f16 mode only (single_pass): the pair tensor stored as f16 -- z_in / z_out then point to [B*L*L,64] f16 (same element order).
     * z_out_f16 alone (block 0: fp32 edge embedding in, f16 out) or both. */
    int z_in_f16, z_out_f16;
    /* optional (persistent kernel, with bias_out): also emit the NEXT block's pair values W_dz z' (down_z, ipa_pytorch.py:440,
     * WITHOUT its bias) as dz_out [B*L*L,16] fp32, so that the next pf_ipa_attn_fwd (its `dz`) reads 64 bytes per pair instead
     * of the 256 of z'.  wb_frags then holds 6 KiB: the 2 fragment pairs of [linear_b (8 rows); down_z rows 0..7] followed by
     * rows 8..15 of down_z as 2 half fragments (pepflowww_amd.engine.pack_bias_frags(w_b, w_dz)).  Skipped tiles (tile_list)
     * are not touched: the caller keeps them zeroed. */
    float* dz_out;
    int dz_out_f16;                /* f16 mode only (single_pass): dz_out points to [B*L*L,16] f16 */
    /* optional: the same 256 KiB of weights packed for the 32x32x16 matrix instruction (pepflowww_amd.engine.pack_et_stream32:
     * 128 entries of [32 features x 16 K] hi | lo fragments in execution order) and the next block's [linear_b; down_z] tile in
     * that form (pack_bias_frags32, 8 KiB; needed with bias_out).  When w_stream32 is set and no dump_* is requested, the 32x32
     * kernel runs (csrc/edge_transition_v4.hip: tiles of 16 rows x 16 columns, pf_edge_transition_v4_tile_rows() for the work
     * list); everything else about the call is unchanged. */
    const void* w_stream32; const void* wb_frags32;
    /* optional (with the dumps): the ReLU gates [h1 > 0] / [h2 > 0] as one bit per (pair, feature), [B*L*L,24] bytes each: byte
     * 4 t + g of a pair holds the features 32 t + 16 h + 4 g + e at bit 4 h + e (t < 6, g < 4, h < 2, e < 4).  pf_et_bwd_chain
     * (m1 / m2) gates with them instead of reading the 768-byte activations back. */
    unsigned char* dump_m1; unsigned char* dump_m2;
    /* optional (32x32 kernel, fp32 pair tensor, L % 16 == 0; ABI 52): z_in / z_out in the kernel's FRAGMENT ORDER instead of
     * [B,L,L,64] -- the pair tensor between two EdgeTransition launches is read by nobody else (the attention takes bias_out / dz_out),
     * so the kernel may keep it in the order its lanes hold it: block ((b, 16 x 16 tile, wave w, 32-pair row pair) = 8 KiB) x piece k
     * (1 KiB) x lane (16 bytes), lane (rl, jl, g) = g * 32 + rl * 16 + jl of pair (i, j) = (16 ib + 2 w + rl, 16 jb + jl), piece k =
     * 4 mt + q holding channels 32 mt + 8 q + 4 g .. + 3.  Every load / store instruction of the pair tensor is then one contiguous
     * KiB (as [.., 64] rows an instruction touched 32 rows, 32 bytes of each).  w_stream32 must then have been packed with the
     * matching K order of the z operand (pepflowww_amd.engine.pack_et_stream32(..., z_frag=True)); pepflowww_amd.engine.z_to_frag /
     * z_from_frag convert a tensor.  Not with tile_list-skipped layouts other than whole tiles (the list is per tile anyway). */
    int z_in_frag, z_out_frag;
    /* optional (ABI 59; fp32-parity mode with z_in_frag / z_out_frag and bias_out, 32 <= L <= 4096): the same 256 KiB of weights in the
     * execution order of the hand-scheduled kernel (csrc/edge_transition_v5.hip: one 512-register wave per SIMD, every fragment
     * feeding 64 pairs, GEMM2 K-outer) -- pepflowww_amd.engine.pack_et_stream64(..., z_frag=True).  When set and the call has that
     * form, that kernel runs; any other form of call falls through to w_stream32 / w_stream as before.  Same inputs, outputs and
     * work-list semantics; results differ from the 32x32 kernel's only by the summation order inside the fp32 accumulators.
     * f16 mode (single_pass with z_in_f16 / z_out_f16 / dz_out_f16 and the frag flags): w_stream64 = the hi planes only (128 KiB,
     * pack_et_stream64(..., f16=True)) and the f16 pair tensor in THAT kernel's fragment order (pepflowww_amd.engine.z16_to_frag64: block
     * (tile, 32-pair group) of 4 KiB = K-step (1 KiB) x lane (the 8 halves of its MFMA operand)) -- not the 16x16x32 kernel's: a
     * single_pass call with w_stream64 set that the kernel does not cover is REFUSED (PF_E_BADARG) instead of falling through. */
    const void* w_stream64;
} pf_edge_transition_args;
int pf_edge_transition_fwd(const pf_edge_transition_args* a, pf_stream_t stream);
int pf_edge_transition_tile_rows(int single_pass);   /* rows i per tile of the persistent kernel (8; 16 in the f16 mode) */
int pf_edge_transition_v4_tile_rows(void);           /* ... of the 32x32 kernel (16) */

/* ---- encode(): once-per-call context featurisation (FlowModel.encode, flow_model.py:75-93) -------
 * node features: NodeEmbedder.forward up to the MLP input (node.py:35-99): aa embedding, per-aa-type
 * local heavy-atom coordinates, backbone dihedral code; plus the ground-truth frames
 * construct_3d_basis(CA, C, N) (geometry.py:89-111).  feat row = 1157 values padded to 1168;
 * the 4-layer MLP (node.py:20-25,101-102) then runs through pf_linear_fwd. */
typedef struct {
    const int64_t* aa; const int64_t* res_nb; const int64_t* chain_nb;  /* [B*L] */
    const float* pos;          /* [B*L,15,3] */
    const float* mask_atoms;   /* [B*L,15] 0/1 */
    const float* gen_mask;     /* [B*L] */
    const float* aa_table;     /* node_embedder.aatype_embed.weight [22,128] */
    const float* freq3;        /* dihed_embed.freq_bands [6] */
    float* feat;               /* [B*L,1168] */
    float* rot1; float* trans1;/* [B*L,9], [B*L,3] ground-truth frames */
    float* mres; float* ctx;   /* [B*L] residue mask (CA present), context mask (CA present & !generate) */
    int B, L;
    int sample_structure, sample_sequence;   /* cfg.interpolant flags (flow_model.py:86-87) */
    /* (ABI 65) residues per sample of the CALLER's batch when the launch runs at another length (0 = L): the dihedral mask
     * structure_mask & roll(+1) & roll(-1) of node.py:86-93 wraps over the caller's residue axis -- residue 0's wrapped neighbour is
     * the caller's residue L0 - 1 (caller padding = False when L0 - 1 >= L, a batch cut to a length bucket), residue L0 - 1's is
     * residue 0; rows L0 .. L - 1 of a launch padded up are padding. */
    int L0;
} pf_node_feat_args;
int pf_node_features_fwd(const pf_node_feat_args* a, pf_stream_t stream);

/* edge features + all five Linears of EdgeEmbedder.forward (edge.py:39-111) fused; 64 pairs per
 * workgroup, the [B,L,L,225] distance tensor never leaves LDS.  w_d0 is distance_embed.0.weight
 * padded to [64,240], w_o0 is out_mlp.0.weight padded to [64,224] (MFMA K granularity). */
typedef struct {
    const int64_t* aa; const int64_t* res_nb; const int64_t* chain_nb;
    const float* pos; const float* mask_atoms;
    const float* ctx; const float* mres;           /* from pf_node_features_fwd */
    const float* aapair_table;  /* [484,64] */
    const float* relpos_table;  /* [65,64] */
    const float* distcoef;      /* aapair_to_distcoef.weight [484,225] (softplus applied inside) */
    const float* freq3;         /* dihedral_embed.freq_bands [6] */
    const float* w_d0; const float* b_d0; const float* w_d2; const float* b_d2;
    const float* w_o0; const float* b_o0; const float* w_o2; const float* b_o2; const float* w_o4; const float* b_o4;
    float* out;                 /* [B,L,L,64] */
    int B, L;
    int sample_structure, sample_sequence;
    /* optional (training path): intermediates the backward needs, per pair: Gaussian features [225], distance_embed.0 output
     * [64], the 224-wide concat tile, out_mlp.0 / .2 outputs [64].  dump_d2 is no longer written (ABI 48): pf_edge_distcoef_bwd
     * takes the squared distances from the features themselves; the field keeps the struct layout. */
    float* dump_g; float* dump_d2; float* dump_h1; float* dump_cat; float* dump_o1; float* dump_o2;
    /* optional workspace of 484*225 floats: when set, softplus(distcoef) is tabulated there first (one small launch) and the pair
     * kernel reads the table instead of evaluating log1p(exp(.)) per (pair, atom pair) -- same values */
    float* softplus_ws;
} pf_edge_feat_args;
int pf_edge_features_fwd(const pf_edge_feat_args* a, pf_stream_t stream);

/* ---- sampler state, flow_model.py:229-374 ------------------------------------------------
 * Device-resident sampler: the loop never syncs with the host.  `step` is a device counter so
 * that one captured hipGraph can be replayed for every step. */
typedef struct {
    /* ground truth / context (from encode) */
    const float* rot1; const float* trans1; const float* ang1; const int64_t* seq1;
    const float* gen_mask;         /* [B*L] 1 = generated residue */
    const float* res_mask;         /* [B*L] */
    /* current state (updated in place) */
    float* rot_t; float* trans_t; float* ang_t; int64_t* seq_t; float* simplex_t;
    /* initial noise kept for the Euler step (flow_model.py:318,328) */
    float* trans0; float* simplex0;
    /* network outputs of this step */
    const float* pred_rot; const float* pred_trans; const float* pred_ang_raw; const float* pred_logits;
    /* trajectory buffers [num_steps, ...]; slot `*step` is written */
    float* traj_rot; float* traj_trans; float* traj_ang; int64_t* traj_seq; float* traj_simplex;
    /* time grid ts[num_steps] (torch.linspace(1e-2,1,N), flow_model.py:280) */
    const float* ts; int num_steps;
    int* step;                     /* device int[2]: [0] step counter, [1] workgroup ticket of pf_sampler_step (zero between calls) */
    float* t_out;                  /* [B] time fed to the next network call */
    /* categorical noise: expo != NULL -> caller-supplied Exp(1) draws [2*num_steps,B*L,20];
     * NULL -> in-kernel Philox4x32-10 keyed by (seed, first_sample+b, draw, residue, class) */
    const float* expo; uint64_t seed; int64_t first_sample;
    int B, L;
    int sample_bb, sample_ang, sample_seq;
    /* optional: device uint64[2] = {seed, first_sample} read at run time (overrides the two fields above), so that the
     * hipGraph captured for one sample() call is replayed by the next call with another seed / shard offset */
    const uint64_t* seed_dev;
    /* optional (ABI 56): device int64 [B] = the GLOBAL index of each local sample (overrides first_sample + b).  A batch that was
     * re-ordered on the way in -- the length buckets of a ragged batch (pepflowww_amd/buckets.py) -- then draws exactly the streams
     * of the unpermuted run: the Philox key is (seed, sample_ids[b], draw, residue, class). */
    const int64_t* sample_ids;
} pf_sampler_args;
/* initial state from raw noise (flow_model.py:252-277): rot0/trans0_raw/ang0/simplex0_raw as drawn */
int pf_sampler_init(const pf_sampler_args* a, const float* rot0, const float* trans0_raw,
                    const float* ang0, const float* simplex0_raw, pf_stream_t stream);
/* post-process the prediction (291-312), record it, then Euler step (316-343) unless last step;
 * increments *step */
int pf_sampler_step(const pf_sampler_args* a, pf_stream_t stream);
/* ---- conditioned sampling: partial start and per-residue constraints -----------------------
 * The reference has NO such call (its sample(), flow_model.py:229-374, always starts from noise and applies its three switches to
 * the whole peptide).  A partial start re-uses the interpolants of the TRAINING corruption (flow_model.py:125-158) to place the
 * initial state between the drawn noise and a given state at time t0 = ts[0]: an off-label use of the trained flow.
 * "Flag" below = the row's bit where res_flags is set, a->sample_* otherwise; it stands in exactly the expressions where
 * pf_sampler_init / pf_sampler_step use a->sample_* (so a constant byte plane equals the scalar flags on every row).
 * init, on a generated row whose flag is on, with partial:
 *   trans_t = (1 - t0) * trans0 + t0 * start_trans          rot_t = geodesic(base = rot0, target = start_rot, t0)
 *   ang_t = torus geodesic(ang0, start_ang, t0)              simplex_t = (1 - t0) * simplex0 + t0 * simplex_of(start_seq)
 *   seq_t = draw 0 from simplex_t
 *   (trans0 / simplex0, which the Euler steps subtract, stay the centred / scaled NOISE; no torsion mask at init, as in 262-267).
 * aa_allowed: classes outside a row's set take no part in ANY categorical draw of that row (maximum, softmax sum, arg-max).
 * cond == NULL, or partial = 0 with NULL planes: the bits of pf_sampler_init / pf_sampler_step. */
typedef struct {
    /* partial start: state interpolated between the drawn noise and this state at time ts[0] */
    int partial;                   /* 0 = the state is the noise, as pf_sampler_init */
    const float* start_rot;        /* [B*L,9]  read on generated rows only; required when partial */
    const float* start_trans;      /* [B*L,3] */
    const float* start_ang;        /* [B*L,5] */
    const int64_t* start_seq;      /* [B*L]   */
    /* per-residue constraints, each optional */
    const uint8_t* res_flags;      /* [B*L] bit0 backbone, bit1 angles, bit2 sequence; NULL = a->sample_* on every row */
    const uint32_t* aa_allowed;    /* [B*L] bit k: class k may be drawn on this row; NULL = all 20 */
} pf_sampler_cond_args;
int pf_sampler_init_cond(const pf_sampler_args* a, const pf_sampler_cond_args* c, const float* rot0, const float* trans0_raw,
                         const float* ang0, const float* simplex0_raw, pf_stream_t stream);
/* pf_sampler_step with the row's flags and allowed classes; ts may be any strictly increasing grid */
int pf_sampler_step_cond(const pf_sampler_args* a, const pf_sampler_cond_args* c, pf_stream_t stream);

/* ---- guided sampling: C-alpha potentials that steer the translation prediction (csrc/guidance.hip) ----------
 * The reference has NO such call, and the trained flow has never seen a shifted prediction: an off-label use, like the partial start.
 * The potentials play the role of RFdiffusion's guiding potentials; they are written here from the formulas below and are not checked
 * against any other program.  Nothing was tuned on a trained checkpoint.
 * One launch between the network and pf_sampler_step*: it writes a GUIDED copy of pred_trans, which the step kernel is then pointed at.
 * Row classes of sample b (positions in Angstrom): movable M = gen_mask & res_mask & backbone flag (res_flags bit 0 when the plane is
 * given, sample_bb otherwise), x = pred_trans there; every other row with res_mask has x = trans1; rows without res_mask take no part.
 * P = gen_mask & res_mask (peptide), C = res_mask & ~gen_mask (context), H = hotspots & C.  With d_ij = |x_i - x_j|, terms in this order:
 *   0 receptor_clash  w0 * sum_{i in P, j in C} max(0, r_receptor - d_ij)^2
 *   1 self_clash      w1 * sum_{i < j in P, j - i >= min_sep} max(0, r_self - d_ij)^2
 *   2 ca_bond         w2 * sum_{l, l+1 in P} max(0, |d - 3.8| - bond_tol)^2
 *   3 hotspot         w3 * sum_{j in H} max(0, s_j - r_hotspot)^2,  s_j = -(1/beta) ln sum_{i in P} exp(-beta d_ij) (evaluated with the
 *                     minimum subtracted; 0 when P is empty or beta <= 0)
 *   4 restraint       sum_p w_p * [max(0, lo_p - d)^2 + max(0, d - hi_p)^2] over the sample's PF_GUIDE_MAX_PAIRS row pairs (either end
 *                     peptide or context; w_p = 0 pads the list; a pair with an end outside res_mask takes no part)
 * g_i = dE/dx_i on M, 0 elsewhere (a pair with d < 1e-6 gives its energy and no gradient).  t = ts[*step] (or t[b]),
 * u = (t - t_on) / (1 - t_on), lambda = 0 for t < t_on, else scale * u^power (power 0, 1 or 2; power 0 = 1);
 * shift_i = lambda g_i * min(1, max_shift / max(|lambda g_i|, 1e-12)); guided_trans_i = float(x_i - shift_i) on M, the bits of
 * pred_trans on every other row -- and on a movable row whose shift is zero.
 * Energies and gradients are accumulated in double, every sum in a fixed order, no atomics: two runs give the same bits.
 * params (device float [PF_GUIDE_NPARAMS]): w0 w1 w2 w3 | r_receptor r_self min_sep bond_tol | r_hotspot beta scale t_on | power
 * max_shift 0 0.  Everything the potentials depend on is read from device memory at run time: a captured graph serves later calls
 * that rewrite the buffers' contents.
 * Sampler mode (step != NULL): slot *step of energy [num_steps,B,5] and shift_max [num_steps,B] is written; *step >= num_steps returns
 * without writing, as pf_sampler_step does.  Stand-alone mode (step == NULL): t [B], energy [B,5]; guided_trans, shift_max and grad
 * (g, unscaled) are each optional.
 * L > PF_GUIDE_MAX_L -> PF_E_TOOLARGE.  The restraint list lives in device memory, so it is the KERNEL that refuses an index outside
 * [0, L): the pair takes no part and error[b] is set to -1 (the kernel never clears it). */
#define PF_GUIDE_MAX_PAIRS 64
#define PF_GUIDE_MAX_L 1024
#define PF_GUIDE_NPARAMS 16
#define PF_GUIDE_NTERMS 5
typedef struct {
    const float* pred_trans;       /* [B*L,3] the network's translation prediction */
    const float* trans1;           /* [B*L,3] context translations */
    const float* gen_mask;         /* [B*L] 1 = generated residue */
    const float* res_mask;         /* [B*L] */
    const uint8_t* res_flags;      /* optional [B*L]: bit 0 = backbone flag of the row (pf_sampler_cond_args.res_flags) */
    const uint8_t* hotspots;       /* optional [B*L]: 1 = hot-spot residue (context rows only) */
    const int* pair_idx;           /* optional [B,PF_GUIDE_MAX_PAIRS,2] residue indices of the restraints */
    const float* pair_par;         /* [B,PF_GUIDE_MAX_PAIRS,3] lo, hi, weight; required with pair_idx */
    const float* params;           /* [PF_GUIDE_NPARAMS] */
    const float* ts;               /* sampler mode: time grid [num_steps] */
    const int* step;               /* sampler mode: device step counter (pf_sampler_args.step); NULL = stand-alone */
    const float* t;                /* stand-alone mode: [B] */
    float* guided_trans;           /* [B*L,3] */
    float* energy;                 /* [num_steps,B,5] / [B,5]: the terms of the UNGUIDED prediction */
    float* shift_max;              /* [num_steps,B] / [B]: the largest |shift_i| of the sample */
    float* grad;                   /* optional, stand-alone mode: [B*L,3] */
    int* error;                    /* optional [B] */
    int B, L, num_steps, sample_bb;
} pf_guidance_args;
int pf_guidance_fwd(const pf_guidance_args* a, pf_stream_t stream);

/* ---- tempered and stochastic sampling: sequence temperature and noise on the backbone state (csrc/temper.hip) ----------
 * The reference has NO such call: its sample() draws every residue type at temperature 1 and integrates the rotation and translation
 * tracks as a deterministic Euler ODE.  The trained flow has never seen a perturbed state: an off-label use, like the partial start and
 * the guidance.  Nothing was tuned on a trained checkpoint.
 * One launch per step, after the network (and after pf_guidance_fwd) and before pf_sampler_step*; one thread per row.  With
 * s = step[0] it returns without writing when s >= num_steps, as pf_sampler_step does.  Two independent parts:
 *  a) tau != NULL, every step, the last one included: tempered_logits[row,k] = pred_logits[row,k] / tau[row] for all 20 classes of every
 *     row (a true division: tau = 1 gives back the input's bits).  The caller points pf_sampler_args.pred_logits at tempered_logits, so
 *     only the PREDICTION draw (draw index 1 + 2s: the recorded sequence and the torsion mask) is tempered; the initial draw and the
 *     state draw from simplex_t are the interpolant's and stay as they are.  tau == NULL: nothing is written.
 *  b) params != NULL, only when s < num_steps - 1: Euler-Maruyama noise on the rows with gen_mask > 0.5 whose backbone flag is on
 *     (res_flags bit 0 when the plane is given, sample_bb otherwise: the rule of pf_sampler_step_cond).  t = ts[s], dt = ts[s+1] - ts[s],
 *     a = sqrtf(dt) * (1 - t)^power for t < t_off, 0 otherwise (power 0, 1 or 2, by multiplication), z = six standard normals of the row:
 *       trans_t += (sigma_trans * a) * z[0:3]              (Angstrom per sqrt of flow time)
 *       rot_t    = rot_t * Exp((sigma_rot * a) * z[3:6])   (radian per sqrt of flow time; a Gaussian in the tangent space, NOT IGSO3)
 *     A part whose scale is 0 leaves its tensor's bits.  The step kernel then takes its Euler step from the perturbed state ("perturb,
 *     then drift").  No other row and no other tensor (trans0, simplex_t, ang_t, seq_t) is touched.
 * z: gauss != NULL -> caller-supplied [num_steps-1,B,L,6]; NULL -> Philox4x32-10 with the sampler's key (seed / seed_dev / sample_ids /
 * first_sample exactly as pf_sampler_args), counter {l*2 + q, 0x80000000 | s, lo32(gs), hi32(gs)} for q in {0, 1} (the categorical
 * draws use counter[1] < 2*num_steps + 1: the high bit keeps the streams apart), uniforms u = ((c >> 8) + 0.5) * 2^-24, Box-Muller
 * r = sqrtf(-2 logf(u_a)), (r cosf(2 pi u_b), r sinf(2 pi u_b)) on the pairs (u0,u1), (u2,u3) of block 0 and (u0,u1) of block 1.
 * params (device float [PF_TEMPER_NPARAMS]): sigma_trans sigma_rot power t_off 0 0 0 0, read at run time: a captured graph serves
 * later calls that rewrite the buffer.
 * PF_E_BADARG: a NULL struct, step or ts, sizes <= 0; neither tau nor params (nothing to do); tau without pred_logits / tempered_logits;
 * params without rot_t / trans_t / gen_mask; gauss without params. */
#define PF_TEMPER_NPARAMS 8
typedef struct {
    /* logits */
    const float* pred_logits;      /* [B*L,20] the network's logits */
    float* tempered_logits;        /* [B*L,20] required with tau */
    const float* tau;              /* optional [B*L] temperature of the row, > 0 */
    /* state */
    float* rot_t;                  /* [B*L,9] */
    float* trans_t;                /* [B*L,3] */
    const float* gen_mask;         /* [B*L] 1 = generated residue */
    const uint8_t* res_flags;      /* optional [B*L]: bit 0 = backbone flag of the row (pf_sampler_cond_args.res_flags) */
    /* time */
    const float* ts;               /* time grid [num_steps] */
    const int* step;               /* device step counter (pf_sampler_args.step) */
    /* noise */
    const float* params;           /* optional [PF_TEMPER_NPARAMS]; NULL = no noise */
    const float* gauss;            /* optional [num_steps-1,B*L,6] standard normals; NULL = in-kernel Philox */
    const uint64_t* seed_dev;      /* optional, as pf_sampler_args.seed_dev */
    const int64_t* sample_ids;     /* optional [B], as pf_sampler_args.sample_ids */
    uint64_t seed;
    int64_t first_sample;
    int B, L, num_steps, sample_bb;
} pf_sampler_temper_args;
int pf_sampler_temper(const pf_sampler_temper_args* a, pf_stream_t stream);

/* ---- steered sampling: on-device particle resampling by guidance energy (csrc/steer.hip) --------------------------------
 * The reference has NO such call.  Feynman-Kac steering (Singhal et al. 2025): sequential Monte Carlo over the samples of one complex
 * (a particle GROUP) with a difference potential on the predicted clean sample and adaptive systematic resampling (Kitagawa 1996;
 * Douc & Cappe 2005).  Written from the publications, not checked against any other program.  Off-label like the guidance and the
 * tempering: nothing was tuned on a trained checkpoint.
 * Two launches, called once per step AFTER pf_sampler_step*: that kernel has bumped the counter, so s = step[0] - 1; both kernels return
 * without writing when s < 0 or s >= num_steps.  B workgroups are launched; workgroup g >= n_groups[0] returns.  Group g has the members
 * m_0 < ... < m_{n-1} = members[group_ptr[g] .. group_ptr[g+1]), n <= PF_STEER_MAX_GROUP.  The structure lives in device memory, so the
 * caller states its largest group in max_group: above PF_STEER_MAX_GROUP -> PF_E_TOOLARGE; a kernel that meets a group outside these
 * limits or a member outside [0, B) leaves that group alone (its slots keep the ancestors the caller initialised: the identity).
 * DECIDE, one workgroup of 256 threads per group, double arithmetic, every sum on one thread in ascending member order, no atomics (two
 * runs give the same bits).  params (device double [PF_STEER_NPARAMS]): lam every ess_frac t_on t_off 0 0 0, read at run time.
 *   E_b = (double)e[s,b,0] + e[s,b,1] + e[s,b,2] + e[s,b,3] + e[s,b,4], summed in that order from the fp32 terms pf_guidance_fwd wrote
 *   for step s (the weighted terms of the UNGUIDED prediction).
 *   The step is ACTIVE when t_on <= (double)ts[s] <= t_off.  Active: logw_b += -lam * (E_b - eprev_b), then eprev_b = E_b (eprev starts
 *   at 0, so the product of the potentials telescopes to exp(-lam E) of the last active step); a non-finite E_b sets logw_b = -inf and
 *   leaves eprev_b; a NaN log-weight counts as -inf.  Inactive: nothing changes.
 *   A resampling MOMENT is an active step with s < num_steps - 1 and (s + 1) % every == 0.  M = max logw; M not finite at a moment ->
 *   code -1, nothing changes.  w_i = exp(logw_i - M), S = sum w_i, Q = sum w_i^2, ESS = S^2 / Q (recorded on every step with a finite
 *   M, else 0).  At a moment the group is resampled iff ess_frac >= 1 or ESS <= ess_frac * n (ess_frac = 0 never does).
 *   Systematic resampling with ONE uniform u per (step, group): p_k = (u + k) / n, a_k = the first i whose raw running sum
 *   C_i > p_k * S (rounding left none: the last i with w_i > 0), c_i = #{k : a_k = i}.  Stable assignment: a slot with c_i >= 1 keeps
 *   its own particle; the dead slots in ascending order receive the list "i repeated c_i - 1 times, i ascending".  Then logw = 0 for the
 *   whole group and eprev of a dead slot becomes its ancestor's.  Sources are surviving slots, destinations dead ones: disjoint sets.
 *   Records of step s: ancestors int32 [num_steps,B] (local sample index; identity when nothing moved), logw_rec double [num_steps,B]
 *   (after the update, before the reset), ess double [num_steps,B] and code int32 [num_steps,B] indexed by GROUP: 0 no moment, 1 a
 *   moment with ESS above the threshold, 2 resampled, -1 degenerate.
 * GATHER, one thread per row of B*L, only when all seven state pointers are given and s < num_steps - 1: a slot b with
 * ancestors[s,b] != b copies row (ancestors[s,b], l) -> (b, l) of rot_t, trans_t, ang_t, seq_t, simplex_t, trans0, simplex0 as raw bits,
 * in place (the disjointness above).
 * u: a caller-supplied double [num_steps,B] indexed by (step, group), or NULL -> Philox4x32-10 with the sampler's key (seed / seed_dev
 * exactly as pf_sampler_args), counter {0, 0xC0000000 | s, lo32(gs0), hi32(gs0)}, gs0 the global sample id of the group's first member
 * (sample_ids[m_0], else first_sample + m_0), u = ((c0 >> 8) + 0.5) * 2^-24.  The categorical draws use counter[1] < 2*num_steps + 1
 * and the temper normals 0x80000000 | s: the two high bits keep the three streams apart.
 * STAND-ALONE (step == NULL): one decision with s = 0 that is always active and always a moment; energy [B,5], logw [B] (in / out),
 * eprev optional (NULL: 0), u [G] or NULL, ancestors [B], ess [G], code [G]; logw_rec [B] optional; ts unused.
 * PF_E_BADARG: a NULL struct, params, group_ptr, members, n_groups or energy; B, L, num_steps or max_group <= 0; logw, ancestors, ess or
 * code missing; in sampler mode ts, eprev or logw_rec missing; state pointers only partly given. */
#define PF_STEER_NPARAMS 8
#define PF_STEER_MAX_GROUP 1024
typedef struct {
    /* energies and time */
    const float* energy;           /* [num_steps,B,5] pf_guidance_args.energy (stand-alone: [B,5]) */
    const float* ts;               /* time grid [num_steps] */
    const int* step;               /* device step counter (pf_sampler_args.step); NULL = stand-alone */
    const double* params;          /* device [PF_STEER_NPARAMS] */
    /* groups */
    const int* group_ptr;          /* device [B+1] */
    const int* members;            /* device [B] sample indices, ascending inside a group */
    const int* n_groups;           /* device [1] */
    /* weights */
    double* logw;                  /* [B] */
    double* eprev;                 /* [B] */
    /* uniforms */
    const double* u;               /* optional [num_steps,B]; NULL = in-kernel Philox */
    const uint64_t* seed_dev;      /* optional, as pf_sampler_args.seed_dev */
    const int64_t* sample_ids;     /* optional [B], as pf_sampler_args.sample_ids */
    /* records */
    int* ancestors;                /* [num_steps,B] */
    double* logw_rec;              /* [num_steps,B] */
    double* ess;                   /* [num_steps,B] by group */
    int* code;                     /* [num_steps,B] by group */
    /* per-particle state of the step kernel: all seven or none */
    float* rot_t;                  /* [B*L,9] */
    float* trans_t;                /* [B*L,3] */
    float* ang_t;                  /* [B*L,5] */
    int64_t* seq_t;                /* [B*L] */
    float* simplex_t;              /* [B*L,20] */
    float* trans0;                 /* [B*L,3] */
    float* simplex0;               /* [B*L,20] */
    uint64_t seed;
    int64_t first_sample;
    int B, L, num_steps, max_group;
} pf_sampler_steer_args;
int pf_sampler_steer(const pf_sampler_steer_args* a, pf_stream_t stream);

/* stand-alone manifold steps (KAT surface): so3_utils.geodesic_t (500-520) and torus.tor_geodesic_t */
int pf_so3_geodesic(const float* base, const float* target, const float* t, float* out, int n, pf_stream_t stream);
int pf_so3_log(const float* rot, float* rotvec, int n, pf_stream_t stream);
int pf_so3_exp(const float* rotvec, float* rot, int n, pf_stream_t stream);
int pf_torus_geodesic(const float* base, const float* target, const float* t, float* out, int n, pf_stream_t stream);

/* ---- training forward, flow_model.py:111-227 (no autograd; the backward row is next) -------
 * corrupt: t = t_raw*(1-2*min_t)+min_t; generated residues are moved to time t on each manifold
 * (translations 131-134, SO(3) geodesic 136-138, torus geodesic 140-142, simplex + categorical
 * draw 149-155); context residues keep the clean values.
 * losses: trans / rot-vf / idealised-backbone / cross-entropy / angle-vf / torsion (161-227),
 * losses[6] in that order = mean over samples of per_sample[B,6]. */
typedef struct {
    /* clean data (from encode) */
    const float* rot1; const float* trans1; const float* ang1; const int64_t* seq1;
    const float* gen_mask; const float* res_mask;     /* [B*L] */
    /* raw noise as drawn: t_raw [B] U[0,1), rot0 [B*L,9], trans0_raw [B*L,3], ang0 [B*L,5], simplex0_raw [B*L,20] */
    const float* t_raw; const float* rot0; const float* trans0_raw; const float* ang0; const float* simplex0_raw;
    /* categorical noise: expo != NULL -> Exp(1) draws [2,B*L,20] (0: seq_t, 1: predicted seq); NULL -> Philox */
    const float* expo; uint64_t seed; int64_t first_sample;
    /* corrupted state (written by corrupt, read by losses) */
    float* t; float* rot_t; float* trans_t; float* ang_t; int64_t* seq_t;
    /* network prediction (losses only); pred_ang_raw = angle_net output before the % 2pi of ga.py:125 */
    const float* pred_rot; const float* pred_trans; const float* pred_ang_raw; const float* pred_logits;
    /* outputs of losses */
    int64_t* pred_seq;            /* [B*L] drawn sequence (optional, may be NULL) */
    float* per_sample;            /* [B,6] */
    float* losses;                /* [6] */
    int B, L;
    int sample_structure, sample_sequence;
    /* optional: the Philox seed read from DEVICE memory at run time (overrides `seed`), so that a training step
     * captured once as a hipGraph draws fresh categorical noise on every replay */
    const uint64_t* seed_dev;
} pf_train_args;
int pf_train_corrupt_fwd(const pf_train_args* a, pf_stream_t stream);
int pf_train_losses_fwd(const pf_train_args* a, pf_stream_t stream);
/* backward of sum_k w[k] * loss_k (train.py:121; weights learn_angle.yaml:37-43, order as losses[6]) with respect
 * to the four network outputs; `a` as passed to pf_train_losses_fwd (pred_seq must have been written by it).
 * First stage of the backward row: the gradients this call produces seed the trunk backward (not built yet). */
typedef struct {
    float w[6];
    float* d_rot;      /* [B*L,9]  d/d pred_rot   */
    float* d_trans;    /* [B*L,3]  d/d pred_trans */
    float* d_ang;      /* [B*L,5]  d/d pred_ang_raw (the % 2pi of ga.py:125 has unit slope) */
    float* d_logits;   /* [B*L,20] d/d pred_logits */
    const float* w_dev; /* optional: the six weights read from device memory (overrides w; graph-captured steps) */
} pf_train_bwd_args;
int pf_train_losses_bwd(const pf_train_args* a, const pf_train_bwd_args* g, pf_stream_t stream);

/* ---- building blocks of the training backward (train.py:133; csrc/backward.hip) -----------------------------
 * Correctness-first fp32 kernels from which the trunk backward is assembled (first users: output heads, final
 * backbone update).  A Linear y = x W^T + b (ipa_pytorch.Linear / nn.Linear) needs three GEMMs:
 *   forward y = x W^T : A = x (sam = ldx, sak = 1), B(k,n) = W[n,k] (sbk = 1, sbn = ldw)
 *   dx = dy W         : A = dy,                     B(k,n) = W[k,n] (sbk = ldw, sbn = 1)      [K = N_out]
 *   dW (+)= dy^T x    : A(m,k) = dy[k,m] (sam = 1, sak = ldy), B = x (sbk = ldx, sbn = 1)     [K = rows] */
typedef struct {
    const float* A; long long sam, sak;
    const float* B; long long sbk, sbn;
    float* C; int ldc;
    int M, N, K;
    int accumulate;                /* C += instead of C = */
    /* optional forward epilogue: C = relu?(alpha A B + bias[n]) + residual[m,n] (residual with C's leading dimension) */
    const float* bias; int relu; const float* residual;
    float alpha;                   /* scale of the product (set 1) */
    /* optional two-level batching (e.g. sample x head): slice (z1, z2) uses A + z1*bsA1 + z2*bsA2 etc.; 0 = no batching */
    int batch1, batch2;
    long long bsA1, bsA2, bsB1, bsB2, bsC1, bsC2;
    int ksplit;                    /* internal (set by the launcher): split-K factor for long-K, few-tile products */
    /* optional (no batching): rowsum_a[m] += sum_k A(m,k), added atomically -- the bias gradient db = column sums of dy falls
     * out of the dW = dy^T x product (A = dy^T) without a pass of its own; must hold zeros or a running sum */
    float* rowsum_a;
    /* optional: C = gate[m,n] > 0 ? C : 0 before the residual is added (gate with C's leading dimension): the ReLU backward of
     * the layer below, fused into dx = dy W */
    const float* gate;
} pf_gemm_args;
int pf_gemm_f32(const pf_gemm_args* a, pf_stream_t stream);
/* the two products of a row-sized Linear backward in ONE launch: dx = dy W (a1) and dW (+)= dy^T x (a2), each described as for
 * pf_gemm_f32.  Their workgroups share a grid (each product alone fills a fraction of the CUs for a chain of global round trips);
 * results are those of two pf_gemm_f32 calls bit for bit, and any pair outside the compiled-in layouts runs as exactly that. */
int pf_gemm_f32_dual(const pf_gemm_args* a1, const pf_gemm_args* a2, pf_stream_t stream);
/* n <= PF_GEMM_GROUP_MAX INDEPENDENT products (no output of one is an operand or the output of another), each described as for
 * pf_gemm_f32, in ONE launch: the batched sample x head products of the IPA backward (ipa_pytorch.py:389-475 reversed: g_q, g_k, g_v
 * and the three point contractions) are short latency chains whose workgroups overlap in a shared grid.  Results are those of n
 * pf_gemm_f32 calls bit for bit; products outside the compiled-in layouts / tile size run as exactly that. */
#define PF_GEMM_GROUP_MAX 6
int pf_gemm_f32_group(const pf_gemm_args* a, int n, pf_stream_t stream);
/* EdgeTransition operands of the TRAINING forward from the fp32 parameters, two launches (the parameters change every step):
 * stream_out = the persistent kernel's 256 KiB fragment stream (pf_edge_transition_args.w_stream: [128][hi 512 | lo 512] f16) as a
 * gather through stream_idx (int32 [128*512] flat indices into trunk.0.weight | trunk.2.weight | final_layer.weight) with
 * lo = f16((w - hi) * lo_scale); pre_w [512,64], pre_b [512] = weight / bias of the per-residue terms a | c | d | e. */
int pf_et_pack_train(const float* w1, const float* b1, const float* w2, const float* wf, const float* bf, const int* stream_idx,
                     void* stream_out, float lo_scale, float* pre_w, float* pre_b, pf_stream_t stream);

/* ---- the dx chain of the EdgeTransition backward in one kernel (csrc/et_bwd.hip; ipa_pytorch.py:233-248 reversed):
 *   g_u = g_y Wf;  g_h2 = g_u * [h2 > 0];  g_h1 = (g_h2 W2) * [h1 > 0];  g_x = g_h1 W1 + g_u
 * g_y [npairs,64] = gradient w.r.t. the pre-LayerNorm output; h1, h2 [npairs,192] = the saved hidden activations
 * (pf_edge_transition_args.dump_h1 / dump_h2); w*T_f16 = the TRANSPOSED weight matrices as fragment-order f16 hi / lo planes
 * (pf_split_pack_f16 with transpose = 1: final_layer [64,192] -> [192,64]; trunk.2 and trunk.0 [192,192]).  Outputs [npairs,192]:
 * g_h2 and g_h1 (already gated: the operands of the weight-gradient products), g_x (for pf_et_concat_bwd).  Same split-precision
 * arithmetic as three pf_linear_fwd products. */
typedef struct {
    const float* g_y; const float* h1; const float* h2;
    const void* wfT_f16; const void* w2T_f16; const void* w1T_f16;
    float* g_h2; float* g_h1; float* g_x;
    long long npairs;
    /* optional: the ReLU gates [h1 > 0], [h2 > 0] as bits, [npairs,24] bytes each (pf_edge_transition_args.dump_m1 / dump_m2); when both
     * are set the kernel reads them instead of h1 / h2 (which may then be NULL): 48 bytes per pair instead of 1536 */
    const unsigned char* m1; const unsigned char* m2;
} pf_et_bwd_args;
int pf_et_bwd_chain(const pf_et_bwd_args* a, pf_stream_t stream);

/* weight gradient of a Linear over all pairs in one pass: C[M,N] (+)= A^T B with A = dy [R,M] (lda), B = x [R,N] (ldb),
 * M <= 192, N <= 256 (multiples of 4), and optionally colsum_a[M] (+)= column sums of A (the bias gradient).  One workgroup owns
 * the whole C for its row range, so A and B are read once (csrc/backward.hip: gemm_tn_wide_kernel; for N <= 192 the product
 * runs on the split-precision f16 MFMA with transposing LDS reads, gemm_tn_split_kernel).  workspace (optional, device memory
 * private to the stream, workspace_elems >= 256 * (M * N + M) floats): the workgroups store their partial sums there and a
 * second kernel adds them up; without it they accumulate with device-scope atomics (~55 us slower at 256 workgroups). */
int pf_gemm_tn_wide(const float* A, int lda, int M, const float* B, int ldb, int N, float* C, int ldc, long long R,
                    int accumulate, float* colsum_a, int colsum_accumulate, float* workspace, long long workspace_elems,
                    pf_stream_t stream);
/* C[M,N] (+)= A^T (B + B2): the same contraction over all R rows with the B operand given as the SUM of two tensors (same ldb), added
 * while a chunk is staged -- final_layer's weight gradient g_y^T (h2 + x) in one pass over g_y (M <= 64, N <= 192, R % 32 == 0). */
int pf_gemm_tn_sum2(const float* A, int lda, int M, const float* B, const float* B2, int ldb, int N, float* C, int ldc, long long R,
                    int accumulate, float* colsum_a, int colsum_accumulate, float* workspace, long long workspace_elems,
                    pf_stream_t stream);   /* colsum_a, workspace: optional, as in pf_gemm_tn_wide */
/* the same two contractions with EdgeTransition's concatenated input x = [z_ij | n_i | n_j] [B L L, 192] gathered from z [B L L, 64] and
 * the per-residue n [B L, 64] while it is staged (x never exists):  C[M,192] (+)= A^T x  (B2 == NULL, M <= 192: trunk.0.weight's
 * gradient, A = the gated g_h1) or  C[M,192] (+)= A^T (B2 + x)  (M <= 64: final_layer.weight's, A = g_y, B2 = h2); L >= 32. */
int pf_gemm_tn_cat(const float* A, int lda, int M, const float* B2, const float* z, const float* n, int B, int L, float* C, int ldc,
                   int accumulate, float* colsum_a, int colsum_accumulate, float* workspace, long long workspace_elems, pf_stream_t stream);
int pf_colsum_f32(const float* x, int ld, int M, int N, float* out, int accumulate, pf_stream_t stream);   /* bias grads */
int pf_relu_bwd(const float* y, float* dy, long long n, pf_stream_t stream);                                /* dy *= (y > 0) */
int pf_relu_gate(const float* y, const float* src, float* dst, long long n, pf_stream_t stream);            /* dst = y > 0 ? src : 0 */
int pf_add_out(const float* a, const float* b, float* dst, long long n, pf_stream_t stream);                 /* dst = a + b */
/* nn.LayerNorm backward over the last dimension (N <= 256, eps 1e-5): dx; dgamma[n] += sum_m dy xhat and dbeta[n] += sum_m dy
 * (optional, both or neither; accumulated atomically per workgroup, so they must hold zeros or a running sum);
 * dgamma_rows[m,n] = dy xhat (optional, the unreduced contributions). */
typedef struct { const float* x; const float* dy; const float* gamma; float* dx; float* dgamma_rows; int M, N;
                 float* dgamma; float* dbeta;
                 /* optional scratch private to the stream (>= (M / 64 + 1) * 2 N floats): pair-sized inputs then write per-workgroup
                  * partial sums that a second kernel adds up, instead of thousands of atomics per column */
                 float* workspace; long long workspace_elems;
                 /* optional: dy[m, :] is multiplied by row_scale[m] on the way in (y * mask in the forward: no masked copy of dy) */
                 const float* row_scale; } pf_layernorm_bwd_args;
int pf_layernorm_bwd(const pf_layernorm_bwd_args* a, pf_stream_t stream);
int pf_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, int M, int N, pf_stream_t stream);
int pf_row_mask(float* x, const float* mask, int M, int N, pf_stream_t stream);        /* x[m,:] *= mask[m] */
int pf_add_inplace(float* dst, const float* src, long long n, pf_stream_t stream);     /* dst += src */
/* backward of the attention core of the sequence transformer (pf_seq_attn_fwd; ga.py:53-62): qkv [B*L,384],
 * g_out [B*L,128] -> g_qkv [B*L,384]; stats = scratch [B*4*L*3] floats.  Probabilities are recomputed. */
int pf_seq_attn_bwd(const float* qkv, const float* mask, const float* g_out, float* g_qkv, float* stats, int B, int L,
                    pf_stream_t stream);
/* reverse of pf_rigid_update_fwd (Rigid.compose_q_update_vec + quat_to_rot, rigid_utils.py:1039-1063,185-205):
 * upstream gradients w.r.t. the NEW rotation matrix / quaternion (optional) / translation -> gradients w.r.t. the
 * update vector [n,6], the old quaternion, the old translation and (optional) the rotation used for the translation
 * update; rot_is_from_quat != 0 folds that last term into g_quat_in (blocks >= 1, where R_old = quat_to_rot(q)). */
typedef struct {
    const float* quat_in; const float* rot_in; const float* upd; int ldu; const float* mask;
    const float* g_rot_out; const float* g_quat_out; const float* g_trans_out;
    float* g_upd; float* g_quat_in; float* g_trans_in; float* g_rot_in;
    int rot_is_from_quat;
    int n;
} pf_rigid_update_bwd_args;
int pf_rigid_update_bwd(const pf_rigid_update_bwd_args* a, pf_stream_t stream);
/* nn.Embedding backward: table_grad[c, :dim] = sum of g[r, :dim] (row stride ldg) over rows with idx[r] == c */
int pf_embedding_bwd(const float* g, int ldg, const int64_t* idx, int rows, int ncls, int dim, float* table_grad, pf_stream_t stream);
/* encoder backward helpers (node.py / edge.py): per-pair indices and masks of EdgeEmbedder.forward (aa-pair class, clamped
 * relative position + 32, same-chain flag, structure-pair mask, residue-pair mask; aa_node = masked residue type per row),
 * embedding-table gradient with atomics and an optional per-row scale, a masked column-slice copy, and the gradient of
 * aapair_to_distcoef through exp(-softplus(w) d^2) (edge.py:83-89). */
int pf_edge_index(const int64_t* aa, const int64_t* res_nb, const int64_t* chain_nb, const float* ctx, const float* mres,
                  int sample_structure, int sample_sequence, int* aap, int* rel, float* same, float* sp, float* mp,
                  int64_t* aa_node, int B, int L, pf_stream_t stream);
int pf_embedding_bwd_atomic(const float* g, int ldg, const int* idx, const float* scale, long long rows, int dim, float* table_grad,
                            pf_stream_t stream);
int pf_slice_relu_mask(const float* src, int lds, int off, const float* ref, int ldr, int off_r, const float* rowscale, float* dst,
                       long long rows, int width, pf_stream_t stream);
/* table_grad [484,225] += d/d aapair_to_distcoef.weight (edge.py:83-89): g_g [pairs, ldg >= 225] = gradient of the Gaussian features,
 * gfeat [pairs,225] = the features themselves (pf_edge_feat_args.dump_g: g = exp(-softplus(w) d2) * mask), aap [pairs] pair-type rows
 * (pf_edge_index), w = the coefficient table, ratio_ws = workspace of 484*225 floats.  The squared distance is taken from the feature
 * itself (-d2 = ln(g) / softplus(w) where g != 0), so the forward does not store it. */
int pf_edge_distcoef_bwd(const float* g_g, int ldg, const float* gfeat, const int* aap, const float* w, float* ratio_ws, long long pairs,
                         float* table_grad, pf_stream_t stream);
/* EdgeTransition in unfused (saved-activation) form for the training path: x [B*L*L,192] = [z_ij | n_i | n_j]
 * (ipa_pytorch.py:236-243), emask [B*L*L] = m_i m_j (optional); and the reverse scatter g_z (+)= g_x[:, :64],
 * g_n [B*L,64] = sum_j g_x[(i,j),64:128] + sum_j g_x[(j,i),128:192]. */
int pf_et_concat(const float* z, const float* n, const float* mask, float* x, float* emask, int B, int L, pf_stream_t stream);
int pf_et_concat_bwd(const float* gx, float* gz, int accumulate_gz, float* gn, int B, int L, pf_stream_t stream);
/* g_quat (+)= (d quat_to_rot(q)/dq)^T g_rot  (rigid_utils.py:185-205): rotation gradients of a block's IPA -> its quaternion */
int pf_quat_to_rot_bwd(const float* quat, const float* g_rot, float* g_quat, int n, int accumulate, pf_stream_t stream);

/* ---- backward of the IPA core (ipa_pytorch.py:389-475; csrc/ipa_bwd.hip), correctness-first -------------------
 * Forward operands as for pf_ipa_attn_fwd; g_feats [B*L,1536] is the gradient w.r.t. its output.  Call order:
 *   pf_ipa_bwd_rows  -> P, gA [B,8,L,L], g_opt [rows,288] (global-frame gradient of o_pt), g_frame_rows [rows,12]
 *                       (d/d trans 3 | d/d rot 9 of the inverse-frame projection), g_gamma_rows [rows,8]
 *   pf_ipa_bwd_pairs -> g_bias [pairs,8], g_pz [pairs,16], g_z [pairs,64] (+= if accumulate_gz)
 *   host GEMMs (pf_gemm_f32, batched over sample x head): g_q = s_qk gA K, g_k = s_qk gA^T Q, g_v = P^T g_o into
 *                       g_proj[:, :3072]; g_vp = P^T g_opt [rows,288]; g_qp [rows,192] = sum_j gA (kp_j - qp_i) (= gA KP, the rows
 *                       of gA sum to zero): written by pf_ipa_bwd_softmax from the differences, or by a product after
 *                       pf_ipa_bwd_rows
 *   pf_ipa_bwd_points -> g_proj[:, 3072:3744] (raw point projections) and += g_frame_rows (point transforms); the key points'
 *                       sum_i gA (qp_i - kp_j) is formed here from gA (g_kp is not read; the field keeps the layout)
 *   pf_ipa_headw_bwd  -> d/d head_weights [8] from the column sum of g_gamma_rows */
typedef struct {
    const float* proj; int ldp; const float* qp; const float* kp; const float* vp; const float* z;
    const float* rot; const float* trans; const float* mask;
    const float* w_b; const float* b_b; const float* w_dz; const float* b_dz; const float* head_w;
    const float* g_feats;
    float* P; float* gA; float* g_opt; float* g_frame_rows; float* g_gamma_rows;
    float* g_bias; float* g_pz; float* g_z; int accumulate_gz;
    float* g_qp; const float* g_kp; const float* g_vp; float* g_proj;
    int B, L;
    /* optional (pf_ipa_bwd_pairs): [pairs,24] = g_bias (8) | g_pz (16) per pair in ONE tensor instead of g_bias / g_pz (which may
     * then be NULL): the parameter gradients of linear_b and down_z (ipa_pytorch.py:352,355) become one [24,64] product over z */
    float* g_bp;
} pf_ipa_bwd_args;
int pf_ipa_bwd_rows(const pf_ipa_bwd_args* a, pf_stream_t stream);
/* the same stage from SAVED probabilities (a->P written by pf_ipa_attn_fwd, p_out) and batched GEMMs issued by the host
 * (pepflowww_amd/backward.py):  pf_ipa_bwd_opt: a->g_opt holds o_pt in the global frame (= P vp) on entry and its gradient
 * on return, + g_frame_rows;  pf_ipa_bwd_pairterm: a->gA (holding g_P so far) += (W_dz^T g_o_pair) . z;
 * pf_ipa_bwd_softmax: a->gA = P (g_P - sum_j P g_P) in place, + g_gamma_rows, + g_qp when given. */
int pf_ipa_bwd_opt(const pf_ipa_bwd_args* a, pf_stream_t stream);
int pf_ipa_bwd_pairterm(const pf_ipa_bwd_args* a, pf_stream_t stream);
int pf_ipa_bwd_softmax(const pf_ipa_bwd_args* a, pf_stream_t stream);
int pf_ipa_bwd_pairs(const pf_ipa_bwd_args* a, pf_stream_t stream);
int pf_ipa_bwd_points(const pf_ipa_bwd_args* a, pf_stream_t stream);
int pf_ipa_headw_bwd(const float* g_gamma, const float* head_w, float* g_head_w, pf_stream_t stream);

/* ---- optimizer step on the device (csrc/optimizer.hip): the block that follows loss.backward() in train.py:135-146 and
 * train_ddp.py:144-155 -- NaN gradient entries count as 0, clip_grad_norm_(max_norm), torch.optim.Adam / AdamW -- over ALL parameter
 * tensors in one call (three launches), with no host read.  Additive to ABI 65.
 *   tables     Everything that describes a step lives in DEVICE memory; only pointers and counts are passed by value, so a captured
 *              launch stays valid when lr (or anything else in a table) changes.
 *                tensors [n_tensors]   pf_optim_tensor: the addresses of the parameter and of its gradient, the offsets (in floats) of
 *                                      its exp_avg / exp_avg_sq into the two flat state buffers, numel, the row of its group, active.
 *                                      A tensor with active == 0 (its gradient is None in this call) is left untouched, counter included.
 *                hyper [(1 + n_groups) * 8]  float64 rows: row 0 = {max_norm, 0...} (max_norm <= 0 or NaN: no clipping), row 1 + g =
 *                                      {lr, beta1, beta2, eps, weight_decay, decoupled (0 = Adam, L2; else AdamW), 0, 0} of group g.
 *                chunks [n_chunks, 2]  (tensor, first element): a chunk is PF_OPTIM_CHUNK consecutive elements of ONE tensor (fewer at
 *                                      its end), first element a multiple of PF_OPTIM_CHUNK; one workgroup handles one chunk.  Every
 *                                      element of every tensor belongs to exactly one chunk.  Entries out of range are ignored.
 *                steps [n_tensors]     int32 step counters, one per tensor as torch keeps them per parameter.
 *   phase 1    per chunk: sum of g^2 over its slice accumulated in float64, NaN entries counted as 0; the NaN count; whether +-inf
 *              was seen.  One partial per chunk into `work`, no atomics.
 *   reduction  one workgroup adds the partials in a fixed order: total_norm = sqrt(sum), coef = min(1, max_norm / (total_norm + 1e-6))
 *              (clip_grad_norm_'s formula, in float64), and advances steps[] of every active tensor by one (one thread per tensor).
 *   phase 2    per element, g = coef * (isnan(g) ? 0 : g), t = the advanced counter, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t in float64:
 *                Adam:  g += wd p            AdamW:  p *= 1 - lr wd
 *                m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g^2;   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 *              with float64 scalars; the moments and the final subtraction are formed in float64 and every stored value is rounded
 *              once; the quotient m / (sqrt(v) / sqrt(bc2) + eps) is formed in fp32 from the rounded moments.
 *   inf guard  if any active gradient holds +-inf the whole update is skipped: parameters, both moments and every counter keep their
 *              bits, result.skipped goes up by one and grad_norm reads +inf.  (torch would turn the inf entries into NaN parameters.)
 *   gradients  are read-only: NaNs are not written back, the clip is applied in registers.
 *   result     {float grad_norm (what clip_grad_norm_ returns), int nan_count, int skipped (running total), int 0}.
 *   alignment  a tensor whose parameter, gradient and both state slices are 16-byte aligned moves in 16-byte accesses, any other
 *              (4-byte aligned) tensor and every tail in 4-byte accesses; the element-to-thread map is the same in both, so the
 *              results are not a function of the alignment.  numel need not be a multiple of 4.
 *   determinism  every word has one writer and every sum one order: bit-identical from run to run; tensors are coupled only through
 *              coef and the inf guard.
 * work: pf_optim_work_bytes(n_chunks) bytes, 16-byte aligned (-1 for n_chunks < 1).  NULL tables, n_tensors / n_groups / n_chunks < 1:
 * PF_E_BADARG. */
#define PF_OPTIM_CHUNK 4096
typedef struct {
    float* param; const float* grad;
    long long exp_avg_off, exp_avg_sq_off;
    int numel, group, active, pad_;
} pf_optim_tensor;
typedef struct {
    const pf_optim_tensor* tensors;
    const double* hyper;
    const int* chunks;
    float* exp_avg; float* exp_avg_sq;
    int* steps;
    void* work;
    int* result;
    int n_tensors, n_groups, n_chunks;
} pf_optim_args;
int pf_optim_step(const pf_optim_args* a, pf_stream_t stream);
int pf_optim_work_bytes(int n_chunks);

/* ---- full-atom reconstruction of sampled residues: models_con/torsion.py:140-226 (+ get_heavyatom_mask 121-138 and
 * the context merge of sample.py:104-108).  Tables: the reference's idealised rigid groups (constants.py), 21 residue
 * types: tab_rot [21,8,9], tab_trans [21,8,3], tab_group [21,14] (int32), tab_pos [21,14,3], tab_mask [22,15] (uint8),
 * frame_group[5] = rigid-group index of psi, chi1..4.  Optional outputs may be NULL. */
typedef struct {
    const float* rot; const float* trans;   /* backbone frames [rows,9], [rows,3] */
    const float* angles;                    /* [rows,5] psi, chi1..4 */
    const int64_t* aa;                      /* [rows] residue types */
    const float* tab_rot; const float* tab_trans; const int* tab_group; const float* tab_pos; const unsigned char* tab_mask;
    int frame_group[5];
    float* pos14;                           /* [rows,14,3] */
    float* frames_rot; float* frames_trans; /* [rows,6,9], [rows,6,3]: backbone, psi, chi1..4 */
    const float* gen_mask; const float* ctx_pos15; float* pos15_merged;   /* where(generate, pad15(pos14), context) */
    unsigned char* mask15;                  /* [rows,15] heavy-atom mask of the residue type */
    int rows;
} pf_full_atom_args;
int pf_full_atom_fwd(const pf_full_atom_args* a, pf_stream_t stream);

/* ---- backbone-only reconstruction: reconstruct_backbone, pepflow/modules/common/geometry.py:446-489 (N, CA, C from the
 * frame and the residue type's idealised coordinates, O from the psi frame with psi = dihedral(N_i, CA_i, C_i, N_{i+1}),
 * 0 at C-termini per topology.py:5-25) and the merge of models_con/sample.py:77-82 (save_samples_bb).
 * tab_bb [21,3,3], tab_o [21,3]: constants.py:878-887.  pos4 / the merged outputs may be NULL (not both). */
typedef struct {
    const float* rot; const float* trans;   /* [B*L,9], [B*L,3] */
    const int64_t* aa; const int64_t* chain_nb; const int64_t* res_nb;   /* [B*L] */
    const unsigned char* mask;              /* [B*L] res_mask */
    const float* tab_bb; const float* tab_o;
    float* pos4;                            /* [B*L,4,3]  N, CA, C, O */
    const float* gen_mask; const float* ctx_pos15; const unsigned char* ctx_mask15;
    float* pos15_merged; unsigned char* mask15;   /* where(generate, pad15(pos4) / first-4 mask, context) */
    int B, L;
} pf_backbone_atoms_args;
int pf_backbone_atoms_fwd(const pf_backbone_atoms_args* a, pf_stream_t stream);

/* ---- evaluation of sampled peptides (ABI 60) ------------------------------------------------------------------------------
 * pf_superpose_fwd: superposition of point sets over a work list, one wave per pair, one launch.  Pair p = (i, j) = pairs[2p],
 * pairs[2p+1] uses the points n with mx[i,n] & my[j,n].  The points are centred first; the cross terms S = X^T Y and the squared
 * norms are accumulated in fp64 and the 3x3 SVD (one-sided Jacobi) runs in fp64.
 *   rmsd_plain[p]  RMSD without superposition;
 *   rmsd[p]        minimal RMSD over proper rotations + translation (Kabsch with reflection correction: Biopython's
 *                  Superimposer.rms), E_x + E_y - 2 (s1 + s2 + sign(det S) s3) clamped at 0;
 *   count[p]       points used; 0 -> every float output of the pair is NaN;
 *   ident[p]       fraction of those points with aa_x[i,n] == aa_y[j,n] (optional, needs aa_x / aa_y);
 *   rot[p] 3x3 row-major, trans[p] 3: y ~ rot x + trans in the mode `allow_reflection` (optional, both or neither):
 *                  1 = r = V U^T from S = U Sigma V^T without determinant correction (pepflow/modules/common/geometry.py:18-56
 *                  align / batch_align), 0 = the proper Kabsch rotation;
 *   aligned[p]     rot x[i,n] + trans for ALL n, masked points included ([P,N,3], optional, needs no rot / trans buffers);
 *   degenerate[p]  1 where S has numerical rank < 2 (s2 <= 1e-6 s1): the rotation is not unique, the identity is returned
 *                  (the RMSDs stay exact); optional.
 * Pair indices outside [0, Bx) x [0, By) are treated as count = 0.  y may alias x. */
typedef struct {
    const float* x; const float* y;                     /* [Bx,N,3], [By,N,3] */
    const unsigned char* mx; const unsigned char* my;   /* [Bx,N], [By,N] */
    const int64_t* aa_x; const int64_t* aa_y;           /* [Bx,N], [By,N] (optional, both or neither) */
    const int* pairs;                                   /* [P,2] */
    float* rmsd_plain; float* rmsd; int* count;         /* [P] */
    float* ident;                                       /* [P] optional */
    float* rot; float* trans;                           /* [P,9], [P,3] optional */
    float* aligned;                                     /* [P,N,3] optional */
    unsigned char* degenerate;                          /* [P] optional */
    int Bx, By, N, P;
    int allow_reflection;
} pf_superpose_args;
int pf_superpose_fwd(const pf_superpose_args* a, pf_stream_t stream);

/* pf_binding_site_fwd: binding-site contacts of eval/geometry.py:93-110 (get_bind_site / get_bind_ratio) on CA coordinates.  For
 * every sample b, the context residues r (res_mask & !gen_mask & ctx_atom_mask[b,r,ca_atom]) with some generated residue p
 * (gen_mask & res_mask) at |ctx_pos[b,r,ca_atom] - pep[b,p]| <= cutoff are marked, once for pep_sample (the sampled CA) and once
 * for pep_native; bsr[b] = |site_sample & site_native| / (|site_native| + 1e-10).  One block per sample. */
typedef struct {
    const float* ctx_pos;                     /* [B,L,n_atoms,3] heavy atoms of the complex */
    const unsigned char* ctx_atom_mask;       /* [B,L,n_atoms] */
    int n_atoms, ca_atom;
    const unsigned char* res_mask; const unsigned char* gen_mask;   /* [B,L] */
    const float* pep_sample; const float* pep_native;               /* [B,L,3] */
    float cutoff;
    unsigned char* site_sample; unsigned char* site_native;         /* [B,L] */
    float* bsr;                                                     /* [B] */
    int B, L;
} pf_binding_site_args;
int pf_binding_site_fwd(const pf_binding_site_args* a, pf_stream_t stream);

/* ---- TM-score with a fixed residue correspondence (ABI 61) ----------------------------------------------------------------
 * pf_tm_score_fwd: the TMscore program's search (Zhang & Skolnick, Proteins 2004) over a work list.  Pair p = (i, j) =
 * pairs[2p], pairs[2p+1] aligns the points n with mx[i,n] & my[j,n], in index order (n_ali of them), and normalises by
 * Lnorm = sum(my[j]): d0 = max(0.5, 1.24 cbrt(Lnorm - 15) - 1.8), score = sum 1 / (1 + (|R x + t - y| / d0)^2) / Lnorm.
 * Seeds: contiguous runs of the aligned list of lengths n_ali, n_ali / 2, ... down to min(4, n_ali), every start; each seed is
 * superposed (proper Kabsch, fp64) and then refined up to 20 times on the points closer than d0_search + 1 (d0_search - 1 after
 * the seed; d0_search = clamp(d0, 4.5, 8); raised by 0.5 until >= 3 points).  The best-scoring superposition is kept, the first
 * one in seed / iteration order on equal scores.
 *   tm[p]          the best score; NaN where n_ali < 3;
 *   count[p]       n_ali (0 for pair indices outside [0, Bx) x [0, By));  lnorm[p]  Lnorm;
 *   rot[p] 3x3 row-major, trans[p] 3: the best transform, y ~ rot x + trans, a proper rotation (optional, both or neither;
 *                  identity / NaN where tm is NaN);
 *   aligned[p]     rot x[i,n] + trans for ALL n, masked points included ([P,N,3], optional; NaN where tm is NaN).
 * One lane per (pair, seed), two launches, no host synchronisation.  `work` is caller-owned scratch of
 * P x pf_tm_score_work_slots(N) x PF_TM_SLOT_BYTES bytes (no initialisation needed).  N > PF_TM_MAX_N -> PF_E_TOOLARGE.  y may alias x.
 * Results are bit-identical from run to run and do not depend on the order or the company of a pair in the work list. */
#define PF_TM_MAX_N 512
#define PF_TM_SLOT_BYTES 112            /* work = P x pf_tm_score_work_slots(N) x PF_TM_SLOT_BYTES bytes */
typedef struct {
    const float* x; const float* y;                     /* [Bx,N,3], [By,N,3] */
    const unsigned char* mx; const unsigned char* my;   /* [Bx,N], [By,N] */
    const int* pairs;                                   /* [P,2] */
    float* tm; int* count; int* lnorm;                  /* [P] */
    float* rot; float* trans;                           /* [P,9], [P,3] optional */
    float* aligned;                                     /* [P,N,3] optional */
    void* work;                                         /* scratch, see above */
    int Bx, By, N, P;
} pf_tm_score_args;
int pf_tm_score_fwd(const pf_tm_score_args* a, pf_stream_t stream);
int pf_tm_score_work_slots(int N);      /* scratch slots per pair (-1 for N outside [1, PF_TM_MAX_N]) */

/* ---- DSSP secondary structure (ABI 62) ------------------------------------------------------------------------------------
 * pf_dssp_fwd: DSSP (Kabsch & Sander, Biopolymers 1983) of B chain slots of N residues, DSSP 2.x conventions (csrc/dssp.hip
 * lists them), geometry in fp64 from the fp32 inputs.  pos [B,N,n_atoms,3] with atoms 0..3 = N, CA, C, O (BBHeavyAtom order, so
 * pos_heavyatom is read as it is; n_atoms >= 4); mask [B,N] the residues taken part; chain [B,N] optional (a change of id breaks
 * the chain); aa [B,N] optional, only to find prolines (aa == pro: not an H-bond donor).
 *   ss [B,N]            8-state codes H 0, B 1, E 2, G 3, I 4, T 5, S 6, '-' 7 (SSTRUCT_SYMB_TO_INDEX of the reference's
 *                       pepflow/modules/protein/dssp.py); 255 where mask is false;
 *   hb_acc [B,N,2]      each donor's two lowest-energy acceptors below 0 kcal/mol (-1: none) and hb_energy [B,N,2] their
 *                       energies (0 with -1); a bond where E < -0.5 (optional, both or neither).
 * One workgroup per slot, one launch, no host synchronisation.  Results do not depend on the other rows and are bit-identical
 * from run to run.  N > PF_DSSP_MAX_N -> PF_E_TOOLARGE.
 * PF_DSSP_PI_PRECEDENCE 1: a pi-helix may overwrite H (DSSP >= 2.1); the older rule leaves H in place. */
#define PF_DSSP_MAX_N 512
#define PF_DSSP_PI_PRECEDENCE 1
typedef struct {
    const float* pos;                   /* [B,N,n_atoms,3] */
    const unsigned char* mask;          /* [B,N] */
    const int64_t* chain;               /* [B,N] optional */
    const int64_t* aa;                  /* [B,N] optional */
    unsigned char* ss;                  /* [B,N] */
    int* hb_acc;                        /* [B,N,2] optional */
    float* hb_energy;                   /* [B,N,2] optional */
    int B, N, n_atoms, pro;             /* pro: the residue index of proline */
} pf_dssp_args;
int pf_dssp_fwd(const pf_dssp_args* a, pf_stream_t stream);

/* ---- TM-align structural alignment (ABI 63) -------------------------------------------------------------------------------
 * pf_tm_align_fwd: TM-align (Zhang & Skolnick, Nucleic Acids Res. 2005) over a work list: a sequence-independent alignment of
 * the CA traces, fp64 from the fp32 inputs.  Pair p = (i, j) = pairs[2p], pairs[2p+1] aligns chain 1 = x[i] on mx[i] (the model,
 * Lx residues in index order) to chain 2 = y[j] on my[j] (the target, Ly residues).  The conventions (search parameters, DP, TM
 * searches, the five initial alignments, the degenerate-fit rule) are listed in csrc/tm_align.hip.
 *   tm[p]          TM-score of the final alignment normalised by Ly (tmtools' tm_norm_chain2); NaN where Lx < 3 or Ly < 3;
 *   tm_x[p]        the same normalised by Lx (tm_norm_chain1);
 *   rmsd[p]        Kabsch RMSD of the n_aligned pairs (NaN when there are none);
 *   n_aligned[p]   aligned pairs within score_d8 under the final superposition (TM-align's n_ali8); 0 for pair indices
 *                  outside [0, Bx) x [0, By); -1 when Lx or Ly exceeds max_len (then every score is NaN);
 *   len_x[p], len_y[p]  Lx, Ly;
 *   rot[p] 3x3 row-major, trans[p] 3: the transform of the search behind tm, y ~ rot x + trans (optional, both or neither;
 *                  identity / NaN where tm is NaN);
 *   y2x[p,n]       for each of y's N positions the aligned position of x (an index into N), -1 unaligned or masked, and kept[p,n]
 *                  1 at the y positions of the n_aligned pairs (optional, both or neither);
 *   aligned[p]     rot x[i,n] + trans for ALL n ([P,N,3], optional).
 * One wave per pair, one launch, no host synchronisation, no scratch.  LDS is sized by max_len, an upper bound on Lx and Ly that
 * the caller may give (0: N); pf_tm_align_lds_bytes(max_len) gives the size (117 KiB at 512).  N > PF_TM_ALIGN_MAX_N ->
 * PF_E_TOOLARGE.  y may alias x.  Results are bit-identical from run to run and do not depend on the rest of the work list. */
#define PF_TM_ALIGN_MAX_N 512
typedef struct {
    const float* x; const float* y;                     /* [Bx,N,3], [By,N,3] */
    const unsigned char* mx; const unsigned char* my;   /* [Bx,N], [By,N] */
    const int* pairs;                                   /* [P,2] */
    float* tm; float* tm_x; float* rmsd;                /* [P] */
    int* n_aligned; int* len_x; int* len_y;             /* [P] */
    float* rot; float* trans;                           /* [P,9], [P,3] optional */
    int* y2x; unsigned char* kept;                      /* [P,N] optional */
    float* aligned;                                     /* [P,N,3] optional */
    int Bx, By, N, P;
    int max_len;                                        /* bound on the compacted lengths, 0: N */
} pf_tm_align_args;
int pf_tm_align_fwd(const pf_tm_align_args* a, pf_stream_t stream);
int pf_tm_align_lds_bytes(int max_len);        /* dynamic LDS of one pair's workgroup (0 for max_len outside [1, PF_TM_ALIGN_MAX_N]) */

/* ---- structural violations (ABI 64) ---------------------------------------------------------------------------------------
 * pf_violations_fwd: AlphaFold's between-residue structural violations (Jumper et al. 2021, Suppl. 1.9.11) of B structures of N
 * residues, with the values of OpenFold's between_residue_clash_loss, between_residue_bond_loss and
 * extreme_ca_ca_distance_violations (openfold/utils/loss.py); the conventions are listed in csrc/violations.hip.
 * pos [B,N,n_atoms,3] in the package's heavy-atom order, n_atoms >= 14, only slots 0..13 are read (pos_heavyatom passes as it is);
 * atom_mask [B,N,n_atoms]; aa [B,N] in the package's numbering; residue_index [B,N]; radius [21,14] van der Waals radii by
 * (type, slot), 0 where the type has no such atom; query [B,N] optional: only atom pairs with an atom in a query residue are
 * evaluated; group [B,N] optional: needed by the *_cross outputs.
 *   clash_atom_loss [B,N,14]   sum of relu(r_a + r_b - clash_overlap_tolerance - d) over the atom's counted partners;
 *   clash_atom [B,N,14]        1 where some counted partner is closer than r_a + r_b - clash_overlap_tolerance;
 *   clash_atom_pairs [B,N,14]  counted partners of the atom;
 *   clash_atom_loss_cross, clash_atom_cross [B,N,14]  the same over partners of another group (optional, both or neither);
 *   clash_mean_loss [B]        summed loss of the unordered pairs / (1e-6 + their number);
 *   bond_c_n_loss_mean, angle_ca_c_n_loss_mean, angle_c_n_ca_loss_mean [B]  masked means over the connections (n, n + 1);
 *   connection_loss [B,N]      half the loss of connection n - 1 plus half that of connection n (not masked, as the reference);
 *   connection_violation [B,N] 1 where connection n - 1 or n violates a bound by more than violation_tolerance_factor stddev;
 *   ca_ca_break [B,N]          1 where CA(n) - CA(n + 1) exceeds 3.802 + 1.5 A (connection n, stored at n);
 *   ca_ca_extreme [B]          breaks / (1e-4 + connections tested).
 * A connection is tested where residue_index[n + 1] - residue_index[n] == 1 and its atoms exist.  The CA-C-N angle test uses the
 * bond-length stddev 0.014 (loss.py:807).  Two launches, no atomics, no scratch, no host synchronisation; memory is O(B N).
 * Results are bit-identical from run to run and do not depend on the other samples.  B > 65535 -> PF_E_TOOLARGE. */
typedef struct {
    const float* pos;                   /* [B,N,n_atoms,3] */
    const unsigned char* atom_mask;     /* [B,N,n_atoms] */
    const int64_t* aa;                  /* [B,N] */
    const int* residue_index;           /* [B,N] */
    const unsigned char* query;         /* [B,N] optional */
    const unsigned char* group;         /* [B,N] optional */
    const float* radius;                /* [21,14] */
    float* clash_atom_loss; unsigned char* clash_atom; int* clash_atom_pairs;       /* [B,N,14] */
    float* clash_atom_loss_cross; unsigned char* clash_atom_cross;                  /* [B,N,14] optional */
    float* clash_mean_loss;                                                         /* [B] */
    float* bond_c_n_loss_mean; float* angle_ca_c_n_loss_mean; float* angle_c_n_ca_loss_mean;   /* [B] */
    float* connection_loss; unsigned char* connection_violation; unsigned char* ca_ca_break;    /* [B,N] */
    float* ca_ca_extreme;                                                           /* [B] */
    int B, N, n_atoms, pro;             /* pro: the residue index of proline */
    float violation_tolerance_factor, clash_overlap_tolerance;      /* AlphaFold: 12.0, 1.5 */
} pf_violations_args;
int pf_violations_fwd(const pf_violations_args* a, pf_stream_t stream);

/* ---- solvent-accessible surface area (ABI 64, added entry point) -------------------------------------------------------------
 * pf_sasa_fwd: Shrake-Rupley solvent-accessible surface of B structures of N residues; the conventions are listed in
 * csrc/sasa.hip.  pos [B,N,n_atoms,3] in the package's heavy-atom order, n_atoms >= 14, slots 0 .. min(n_atoms,15)-1 are read;
 * atom_mask [B,N,n_atoms]; aa [B,N]; radius [21,15] by (type, slot), 0 where the type has no such atom; points [n_points,3] unit
 * vectors, 1 <= n_points <= PF_SASA_MAX_POINTS; work [B,N,4] scratch (per-residue centre and padded extent); query [B,N] optional:
 * only atoms of query residues are evaluated (every existing atom is still a partner); group [B,N] optional: needed by the *_own
 * outputs (all four or none), the same quantities with only atoms of residues of the same group byte as partners.
 *   count [B,N,15]         accessible points of the atom (0: no atom; -1: an atom of a residue outside `query`);
 *   sasa_atom [B,N,15]     4 pi (radius + probe_radius)^2 count / n_points (0 where count <= 0);
 *   sasa_residue [B,N]     sum of sasa_atom over the slots, in slot order;
 *   sasa_total [B]         sum of sasa_atom over the structure, accumulated in fp64.
 * Three launches, no atomics, no host synchronisation; memory is O(B N).  Results are bit-identical from run to run and do not
 * depend on the other samples.  N > PF_SASA_MAX_N or B > 65535 -> PF_E_TOOLARGE. */
#define PF_SASA_MAX_N 512
#define PF_SASA_MAX_POINTS 1024
#define PF_SASA_SLOTS 15
typedef struct {
    const float* pos;                   /* [B,N,n_atoms,3] */
    const unsigned char* atom_mask;     /* [B,N,n_atoms] */
    const int64_t* aa;                  /* [B,N] */
    const unsigned char* query;         /* [B,N] optional */
    const unsigned char* group;         /* [B,N] optional */
    const float* radius;                /* [21,15] */
    const float* points;                /* [n_points,3] */
    float* work;                        /* [B,N,4] scratch */
    int* count; float* sasa_atom;       /* [B,N,15] */
    float* sasa_residue;                /* [B,N] */
    float* sasa_total;                  /* [B] */
    int* count_own; float* sasa_atom_own; float* sasa_residue_own; float* sasa_total_own;       /* optional, all or none */
    int B, N, n_atoms, n_points;
    float probe_radius;                 /* >= 0; 1.4 for water */
} pf_sasa_args;
int pf_sasa_fwd(const pf_sasa_args* a, pf_stream_t stream);

/* ---- cavity detection (ABI 65, added entry points) ----------------------------------------------------------------------------
 * pf_cavity_fwd: a LIGSITE-style buriedness scan (Hendlich et al. 1997) of B structures of N residues over a regular grid, the
 * connected cavities of the buried free points, their ranking and their lining residues (csrc/cavity.hip).  pos [B,N,n_atoms,3]
 * in the package's heavy-atom order, n_atoms >= 14, slots 0 .. min(n_atoms,15)-1 are read; atom_mask [B,N,n_atoms]; aa [B,N];
 * radius [21,15] by (type, slot); origin [B,3]; nx, ny, nz and h are common to the batch, G = nx * ny * nz.  The contract:
 *   Point        linear index i = (ix * ny + iy) * nz + iz; its coordinate is g = origin + (float)index * h per axis, in fp32.
 *   Occupied     for some atom a whose atom_mask is set: ((dx*dx + dy*dy) + dz*dz) <= R_a*R_a with dx = gx - ax, dy = gy - ay,
 *                dz = gz - az, in fp32, in exactly that order, no contraction; R_a = radius[type, slot] + probe, added in fp32.
 *   Buriedness   of a free point, 0..7: the number of the 7 lines through it (the 3 axes, the 4 body diagonals) on which an occupied
 *                point lies within n_axis (axes) / n_diag (diagonals) grid steps in BOTH senses.  A walk ends at the grid's edge:
 *                outside the grid is free.  The caller computes n_axis = floor(max_ray / h), n_diag = floor(max_ray / (h sqrt 3)) in
 *                float64.  An occupied point gets 255.
 *   Cavity point a free point with buriedness >= min_buried (1..7).
 *   Cavities     the connected components of the cavity points under connectivity 6 (faces) or 26 (faces, edges, corners).
 *                Components of fewer than min_points points are dropped; the rest are ranked by size descending, ties by the
 *                smallest linear index of a member; the first max_cavities (1..PF_CAVITY_MAX_OUT) are reported, K = max_cavities.
 *   occupied [B,G]      1 / 0;                 buried [B,G]    the buriedness, 255 where occupied;
 *   label [B,G]         rank of the point's cavity among the reported ones, or -1;
 *   n_found [B]         kept components before the max_cavities cut;
 *   size [B,K]          points of the cavity;
 *   center [B,K,3]      mean of the members' coordinates g, accumulated in double, rounded once;
 *   mean_buried [B,K]   mean buriedness of the members, likewise;
 *   lining [B,K,N]      1 when the residue has an atom (atom_mask set) within r_lining of a member point: ((dx*dx + dy*dy) + dz*dz)
 *                       <= r_lining*r_lining, the same fp32 rule;
 *   rows k >= min(n_found, K) of size, center, mean_buried and lining are zero.
 *   status [1]          0, or a bit set by a device loop that ran out of its bound (1: a path to a root, 2: the retries of a link,
 *                       4: the list of components); the outputs are then not valid.  Every device loop is bounded by the arguments
 *                       (steps of a walk, the grid, G); none waits for another thread.
 * work: B x pf_cavity_work_bytes(nx, ny, nz) bytes, no initialisation needed.  A fixed sequence of launches and memset nodes on the
 * caller's stream, integer atomics only, nothing read back by the host: the results are bit-identical from run to run and do not
 * depend on the other structures.  N > PF_CAVITY_MAX_N, G > PF_CAVITY_MAX_POINTS or B > 65535 -> PF_E_TOOLARGE. */
#define PF_CAVITY_MAX_N 4096
#define PF_CAVITY_MAX_POINTS 2097152    /* 128^3 */
#define PF_CAVITY_MAX_OUT 32
#define PF_CAVITY_SLOTS 15
typedef struct {
    const float* pos;                   /* [B,N,n_atoms,3] */
    const unsigned char* atom_mask;     /* [B,N,n_atoms] */
    const int64_t* aa;                  /* [B,N] */
    const float* radius;                /* [21,15] */
    const float* origin;                /* [B,3] */
    void* work;                         /* B x pf_cavity_work_bytes(nx, ny, nz) bytes */
    unsigned char* occupied; unsigned char* buried;     /* [B,G] */
    int* label;                         /* [B,G] */
    int* n_found;                       /* [B] */
    int* size;                          /* [B,K] */
    float* center;                      /* [B,K,3] */
    float* mean_buried;                 /* [B,K] */
    unsigned char* lining;              /* [B,K,N] */
    int* status;                        /* [1] */
    int B, N, n_atoms, nx, ny, nz, n_axis, n_diag, min_buried, connectivity, min_points, max_cavities;
    float h, probe, r_lining;
} pf_cavity_args;
int pf_cavity_fwd(const pf_cavity_args* a, pf_stream_t stream);
int pf_cavity_work_bytes(int nx, int ny, int nz);   /* scratch bytes per structure (-1 for a dimension < 1 or G > PF_CAVITY_MAX_POINTS) */

/* ---- torsion angles and side-chain packing (ABI 64, added entry points) -------------------------------------------------------
 * pf_torsions_fwd: omega, phi, psi, psi_o (N, CA, C, O) and chi1-chi4 of B structures of N residues; the conventions are listed in
 * csrc/torsions.hip.  pos [B,N,n_atoms,3] in the package's heavy-atom order, n_atoms >= 14, slots 0..13 are read; atom_mask
 * [B,N,n_atoms]; aa [B,N]; residue_index [B,N] optional (absent: consecutive positions are bonded); chi_atoms [21,4,4] the heavy-atom
 * slots of chi1-4 by type, -1 where the type has no such angle.
 *   angles [B,N,8]     radians in [0, 2 pi): omega, phi, psi, psi_o, chi1..chi4; 0 where not defined (never NaN);
 *   defined [B,N,8]    1 where the four atoms are in atom_mask, the neighbour a backbone angle needs is bonded (residue_index grows by
 *                      exactly 1), the type has the chi, and no part perpendicular to the central bond has zero length.
 * psi_o is slot 0 of the reference's get_torsion_angle; on rebuilt coordinates it is the model's first angle + pi.  fp32, atan2 form,
 * from coordinate differences.  One launch, no scratch, no host synchronisation.  angles must be 8-byte and defined 4-byte aligned.
 * B > 65535 -> PF_E_TOOLARGE.
 *
 * pf_sidechain_compare_fwd: for every pair (i, j) of pairs [P,2], x[i] against y[j] residue by residue: wrapped angle errors per slot,
 * residues with every chi within correct_tol, and the deviation of side-chain atoms 4..13 in the residues' own backbone frames.
 * angles_* / defined_* are pf_torsions_fwd's outputs (16- and 8-byte aligned); periodic [21,4]: chi k of the type is pi-periodic;
 * swap [21,4]: two pairs (a1, b1, a2, b2) of equivalent slots of the type, (0, 0) unused.  y may alias x.
 *   err_sum [P,8] (fp64, radians), err_count, within [P,8]   over the residues where both angles are defined (slots 3..7: and the
 *                      types are equal and in 0..19); within counts error <= correct_tol;
 *   res_with_chi, res_correct [P]   residues with a compared chi; those with every compared chi within correct_tol;
 *   sc_sq_sum [P] (fp64), sc_atoms [P], sc_rmsd [P] (NaN when sc_atoms is 0)   squared frame-local deviations, the smaller of the
 *                      plain and the slot-exchanged sum per residue;
 *   err [P,N,8] (NaN: not compared), sc_sq [P,N], sc_n [P,N], swapped [P,N]   optional, all four or none.
 * A pair with an index out of range gives zero counts and NaN.  One launch, a workgroup per pair looping over N, fixed-order sums, no
 * floating-point atomics: bit-identical from run to run and independent of the rest of the list.  N * 8 > INT_MAX -> PF_E_TOOLARGE. */
typedef struct {
    const float* pos;                   /* [B,N,n_atoms,3] */
    const unsigned char* atom_mask;     /* [B,N,n_atoms] */
    const int64_t* aa;                  /* [B,N] */
    const int* residue_index;           /* [B,N] optional */
    const int* chi_atoms;               /* [21,4,4] */
    float* angles;                      /* [B,N,8] */
    unsigned char* defined;             /* [B,N,8] */
    int B, N, n_atoms;
} pf_torsions_args;
int pf_torsions_fwd(const pf_torsions_args* a, pf_stream_t stream);

typedef struct {
    const float* pos_x; const float* pos_y;                         /* [Bx,N,n_atoms_x,3], [By,N,n_atoms_y,3] */
    const unsigned char* mask_x; const unsigned char* mask_y;       /* [Bx,N,n_atoms_x], [By,N,n_atoms_y] */
    const int64_t* aa_x; const int64_t* aa_y;                       /* [Bx,N], [By,N] */
    const float* angles_x; const float* angles_y;                   /* [Bx,N,8], [By,N,8] */
    const unsigned char* defined_x; const unsigned char* defined_y; /* [Bx,N,8], [By,N,8] */
    const int* pairs;                                               /* [P,2] */
    const unsigned char* periodic;                                  /* [21,4] */
    const unsigned char* swap;                                      /* [21,4] */
    double* err_sum; int* err_count; int* within;                   /* [P,8] */
    int* res_with_chi; int* res_correct;                            /* [P] */
    double* sc_sq_sum; int* sc_atoms; float* sc_rmsd;               /* [P] */
    float* err; float* sc_sq; int* sc_n; unsigned char* swapped;    /* [P,N,8], [P,N] x 3: optional, all or none */
    int Bx, By, N, P, n_atoms_x, n_atoms_y;
    float correct_tol;                                              /* radians, >= 0 */
} pf_sidechain_compare_args;
int pf_sidechain_compare_fwd(const pf_sidechain_compare_args* a, pf_stream_t stream);

/* ---- hydrogen bonds and salt bridges (ABI 65, added entry point) -------------------------------------------------------------------
 * pf_polar_fwd: directional hydrogen bonds and salt-bridge atom pairs between the heavy atoms of different residues of a batch of
 * structures, with explicit partner lists; the conventions are listed in csrc/polar.hip.  Heavy-atom criteria written from the
 * publications (Baker & Hubbard 1984, McDonald & Thornton 1994: donor-acceptor distance and antecedent angles; Barlow & Thornton 1983:
 * N-O distance) and checked against a float64 restatement; NOT checked against HBPLUS, PLIP or Rosetta.  Slots 0 .. min(n_atoms, 15) - 1
 * are read; an atom takes part where atom_mask is set and its type has the slot (antecedents[type][slot][0] >= 0: every heavy atom is
 * bonded to another of its residue).  residue_index: consecutive residues of a chain differ by exactly 1.
 *   hbonds_atom, salt_atom [B,N,15]            partners of the row atom (a participating atom that is not a query row: -1);
 *   hbonds_atom_cross, salt_atom_cross         partners whose residue has another group byte;
 *   hbond_partner, salt_partner [B,N,15,4]     residue * 15 + slot of the partners, ascending, the 4 lowest, padded with -1;
 *   hbonds_residue, salt_residue [B,N] (and the _cross twins)   the sums over the slots of the row atoms.
 * The four _cross outputs and group come together or not at all.  Every pair shows in both of its rows; query restricts the rows, not
 * the partners.  work: [B,N,4] floats, no initialisation needed.  Two launches, no atomics, nothing pair-sized, one writer per
 * output: bit-identical from run to run and independent of the rest of the batch.  N > PF_POLAR_MAX_N, n_atoms < 14, a cutoff that
 * is not finite and positive or a cosine outside [-1, 1] -> PF_E_BADARG; B > 65535 -> PF_E_TOOLARGE. */
#define PF_POLAR_MAX_N 512
#define PF_POLAR_MAX_PARTNERS 4
typedef struct {
    const float* pos;                                               /* [B,N,n_atoms,3] */
    const unsigned char* atom_mask;                                 /* [B,N,n_atoms] */
    const int64_t* aa;                                              /* [B,N] */
    const int64_t* residue_index;                                   /* [B,N] */
    const unsigned char* group;                                     /* [B,N] optional */
    const unsigned char* query;                                     /* [B,N] optional */
    const unsigned char* types;                                     /* [21,15] bit 1 donor, bit 2 acceptor */
    const unsigned char* charge;                                    /* [21,15] 0 none, 1 cation N, 2 anion O */
    const signed char* antecedents;                                 /* [21,15,2] bonded slots of the residue, -1: none */
    float* work;                                                    /* [B,N,4] */
    int* hbonds_atom; int* salt_atom;                               /* [B,N,15] */
    int* hbonds_atom_cross; int* salt_atom_cross;                   /* [B,N,15] optional */
    int* hbond_partner; int* salt_partner;                          /* [B,N,15,4] */
    int* hbonds_residue; int* salt_residue;                         /* [B,N] */
    int* hbonds_residue_cross; int* salt_residue_cross;             /* [B,N] optional */
    int B, N, n_atoms;
    float d_max;                                                    /* > 0; 3.5 */
    float cos_acc, cos_don;                                         /* cosines of the smallest angles at the acceptor / donor; 0 */
    float salt_max;                                                 /* > 0; 4.0 */
} pf_polar_args;
int pf_polar_fwd(const pf_polar_args* a, pf_stream_t stream);

/* ---- sequence ratio, pairwise alignment and library search (ABI 65, added entry points) ---------------------------------------------
 * Sequence comparison of peptides of different lengths; the conventions are listed in csrc/seqalign.hip.  The first two take the
 * pair-work-list family of pf_superpose_fwd on residue types: the sequence of side x in pair p = (i, j) is aa_x[i] where mx[i] is set, in
 * order (compacted on the device, N is not bounded), side y likewise from aa_y[j], my[j]; a type outside 0..19 is 20 ("X").  A compacted
 * length above PF_SEQ_MAX_LEN on either side, or a pair index out of range, writes the fill values.  One launch each, no atomics, no
 * scratch, one writer per output, integers but for one float64 division per pair: bit-identical from run to run and independent of the
 * rest of the list.  Every loop of the kernels has a constant trip bound or runs over a size argument.
 *
 * pf_seq_ratio_fwd: difflib.SequenceMatcher(None, x, y) -- matches (the sum of the matching blocks), total = len x + len y and
 * ratio = 2.0 * matches / total in float64 (1.0 when total is 0), the values of the reference's diff_ratio (eval/geometry.py); blocks
 * [P,64,3] / n_blocks [P] (optional, both or neither): get_matching_blocks() without its sentinel, unused rows (-1, -1, 0).
 * Fill: ratio NaN, matches, total, n_blocks -1.
 *
 * pf_seq_align_fwd: Gotoh's affine-gap alignment in int32 with matrix [21,21] (int8); a gap of length g costs
 * gap_open + (g - 1) gap_extend, 0 <= gap_extend <= gap_open <= PF_SEQ_MAX_GAP.  PF_SEQ_GLOBAL penalises end gaps; PF_SEQ_LOCAL is
 * Smith-Waterman (the largest cell, of equal ones the smallest i, then j).  Traceback ties: diagonal, then F (x against a gap), then E;
 * "opened" before "extended".  identity = n_ident / n_columns (NaN without columns); the span [x_lo,x_hi) x [y_lo,y_hi) and x2y [P,64]
 * (optional; -1: a gap or outside the span) are in compacted coordinates.  Fill: score INT_MIN, counts and span -1, identity NaN.
 *
 * pf_seq_search_fwd: each query aa / mask [Q,N] against the library db_aa [D,Ld] (compact, Ld <= 64; an entry with db_len outside
 * [0, Ld] is never the best): the entry of the highest alignment score, of equal scores the lowest index; the Q x D scores are never
 * stored.  A query above PF_SEQ_MAX_LEN, or no valid entry: best_index -1, best_score INT_MIN, counts -1, identity NaN. */
#define PF_SEQ_MAX_LEN 64
#define PF_SEQ_TYPES 21
#define PF_SEQ_MAX_GAP 4096
#define PF_SEQ_GLOBAL 0
#define PF_SEQ_LOCAL 1
typedef struct {
    const int64_t* aa_x; const int64_t* aa_y;                       /* [Bx,N], [By,N] */
    const unsigned char* mx; const unsigned char* my;               /* [Bx,N], [By,N] */
    const int* pairs;                                               /* [P,2] */
    double* ratio;                                                  /* [P] */
    int* matches; int* total; int* len_x; int* len_y;               /* [P] */
    int* blocks; int* n_blocks;                                     /* [P,64,3], [P] optional */
    int Bx, By, N, P;
} pf_seq_ratio_args;
int pf_seq_ratio_fwd(const pf_seq_ratio_args* a, pf_stream_t stream);

typedef struct {
    const int64_t* aa_x; const int64_t* aa_y;                       /* [Bx,N], [By,N] */
    const unsigned char* mx; const unsigned char* my;               /* [Bx,N], [By,N] */
    const int* pairs;                                               /* [P,2] */
    const signed char* matrix;                                      /* [21,21] */
    int* score; int* n_ident; int* n_aligned; int* n_columns;       /* [P] */
    int* x_lo; int* x_hi; int* y_lo; int* y_hi;                     /* [P] */
    int* len_x; int* len_y;                                         /* [P] */
    double* identity;                                               /* [P] */
    int* x2y;                                                       /* [P,64] optional */
    int Bx, By, N, P;
    int mode, gap_open, gap_extend;
} pf_seq_align_args;
int pf_seq_align_fwd(const pf_seq_align_args* a, pf_stream_t stream);

typedef struct {
    const int64_t* aa;                                              /* [Q,N] */
    const unsigned char* mask;                                      /* [Q,N] */
    const int64_t* db_aa;                                           /* [D,Ld] */
    const int* db_len;                                              /* [D] */
    const signed char* matrix;                                      /* [21,21] */
    int* best_index; int* best_score; int* best_n_ident; int* best_n_columns;   /* [Q] */
    double* best_identity;                                          /* [Q] */
    int Q, N, D, Ld;
    int mode, gap_open, gap_extend;
} pf_seq_search_args;
int pf_seq_search_fwd(const pf_seq_search_args* a, pf_stream_t stream);

/* ---- lDDT and interface contacts (ABI 64, added entry points) ------------------------------------------------------------------
 * Both take the work-list family of pf_sidechain_compare_fwd: pair p = (i, j) of pairs [P,2] looks at the model x[i] and the reference
 * structure y[j] (y may alias x); group / query [By,N] belong to y; a pair with an index out of range gives zeros (min_dist: +inf).
 * One launch each (per 65535 pairs), no atomics, no scratch, nothing pair-sized; integer outputs, flags and minima with one writer:
 * bit-identical from run to run, independent of the rest of the batch and of the order of the list.  N > 512 -> PF_E_TOOLARGE.
 *
 * pf_lddt_fwd: the counts of the local distance difference test with the values of OpenFold's `lddt` / `lddt_ca`
 * (openfold/utils/loss.py:382-458); the conventions are listed in csrc/lddt.hip.  Slots 0..13 are read.  An atom is compared when its
 * slot is in slot_mask (0x2: CA, 0xF: N CA C O, 0x3FFF: all), it is set in mask_x[i] and mask_y[j] and, for slots >= 4,
 * aa_x == aa_y at the residue.  A pair of compared atoms is scored when d_y = sqrt(1e-10 + |a - b|^2) < cutoff in y, they are not the
 * same atom and, with exclude_same_residue, not of one residue (0: the reference's behaviour); it adds
 * [|d_y - d_x| < 0.5] + [< 1] + [< 2] + [< 4] to kept.
 *   scored, kept [P,N]                     per row residue, summed over its atoms;
 *   scored_cross, kept_cross [P,N]         partners whose residue has another group byte (optional, both or neither; need group);
 *   scored_atom, kept_atom [P,N,14]        per row atom (optional, both or neither);
 *   scored_atom_cross, kept_atom_cross     (optional, both or neither; need group).
 * With query only rows in query residues are evaluated (the rest 0); every compared atom is still a partner.
 *
 * pf_contacts_fwd: residue contacts across the groups, in x[i] and in y[j] at once (DockQ's Fnat and interface, Basu & Wallner 2016);
 * the conventions are listed in csrc/contacts.hip.  Slots 0 .. min(n_atoms, 15) - 1 in slot_mask are read, each structure on its own
 * atom_mask.  A residue pair (p, q) counts when the group bytes differ and each residue has an atom in x[i] and one in y[j]; m_x, m_y:
 * its minimal squared atom distance in each structure (fp32), compared as m < cutoff^2.
 *   contacts_x, contacts_y, contacts_shared [P,N]   the q in contact (contact_cutoff) in x, in y, in both;
 *   interface_x, interface_y [P,N]                  1 where some q is within interface_cutoff;
 *   min_dist_x, min_dist_y [P,N]                    sqrt of the smallest m over the counted q, +inf without any. */
#define PF_LDDT_MAX_N 512
#define PF_LDDT_SLOTS 14
#define PF_CONTACTS_MAX_N 512
#define PF_CONTACTS_SLOTS 15
typedef struct {
    const float* pos_x; const float* pos_y;                         /* [Bx,N,n_atoms_x,3], [By,N,n_atoms_y,3] */
    const unsigned char* mask_x; const unsigned char* mask_y;       /* [Bx,N,n_atoms_x], [By,N,n_atoms_y] */
    const int64_t* aa_x; const int64_t* aa_y;                       /* [Bx,N], [By,N] */
    const int* pairs;                                               /* [P,2] */
    const unsigned char* group;                                     /* [By,N] optional */
    const unsigned char* query;                                     /* [By,N] optional */
    int* scored; int* kept;                                         /* [P,N] */
    int* scored_cross; int* kept_cross;                             /* [P,N] optional */
    int* scored_atom; int* kept_atom;                               /* [P,N,14] optional */
    int* scored_atom_cross; int* kept_atom_cross;                   /* [P,N,14] optional */
    int Bx, By, N, P, n_atoms_x, n_atoms_y;
    int slot_mask, exclude_same_residue;
    float cutoff;                                                   /* > 0; 15.0 */
} pf_lddt_args;
int pf_lddt_fwd(const pf_lddt_args* a, pf_stream_t stream);

typedef struct {
    const float* pos_x; const float* pos_y;                         /* [Bx,N,n_atoms_x,3], [By,N,n_atoms_y,3] */
    const unsigned char* mask_x; const unsigned char* mask_y;       /* [Bx,N,n_atoms_x], [By,N,n_atoms_y] */
    const int* pairs;                                               /* [P,2] */
    const unsigned char* group;                                     /* [By,N] */
    int* contacts_x; int* contacts_y; int* contacts_shared;         /* [P,N] */
    unsigned char* interface_x; unsigned char* interface_y;         /* [P,N] */
    float* min_dist_x; float* min_dist_y;                           /* [P,N] */
    int Bx, By, N, P, n_atoms_x, n_atoms_y;
    int slot_mask;
    float contact_cutoff, interface_cutoff;                         /* > 0; 5.0, 10.0 */
} pf_contacts_args;
int pf_contacts_fwd(const pf_contacts_args* a, pf_stream_t stream);

/* ---- clustering of samples from a pairwise distance matrix (ABI 64, added entry points) ---------------------------------------------
 * pf_cluster_fwd: the samples of each group clustered on a [B,B] distance matrix (what the pairwise_* functions return: symmetric,
 * NaN across groups); the conventions and the tie rules are listed in csrc/clustering.hip.  index [B] lists the batch indices sorted
 * by group and ascending inside a group, offsets [G+1] the groups' ranges in it; a sample's position is its rank inside its group.
 * For positions a < b only dist[index[a], index[b]] is read, never the mirrored entry or the diagonal; NaN counts as +inf and is
 * never within a cutoff (a cutoff of +inf is taken as FLT_MAX).
 *   method 0  gromos (Daura et al. 1999): repeatedly the active sample with the most active neighbours (d <= cutoff, itself included;
 *             of equal counts the smallest position) and those neighbours leave as the next cluster; the representative is that centre;
 *   method 1, 2, 3  single, complete, average linkage: the pair of clusters with the smallest linkage distance (of equal distances the
 *             smallest (i, j), a cluster named by its smallest position) merges while that distance is <= cutoff; average is
 *             (n_i d_ik + n_j d_jk) / (n_i + n_j) in fp64.  Labels by size descending, then smallest position; the representative is
 *             the medoid (smallest fp64 sum of distances to the other members, summed in ascending position; ties: smallest position).
 *   label, cluster_size, representative, n_neighbours [B] at the sample's batch index; representative and best are batch indices;
 *   best [B] (with score): the member of the own cluster with the lowest score, NaN last, ties to the smallest position;
 *   n_neighbours: the neighbour count over the whole group, itself included (every method);  n_clusters [G].
 * work: G x pf_cluster_work_bytes(n_max, method) bytes (the linkages' working matrix; 0 for gromos, work may then be null), no
 * initialisation needed.  n_max: an upper bound on the group sizes, which sizes the LDS and the scratch stride; a group above it, or
 * offsets / index entries out of range, give n_clusters 0 for that group and nothing else written.  One launch, one workgroup per
 * group, integer outputs with one writer each: bit-identical from run to run and independent of the other groups.
 * n_max > PF_CLUSTER_MAX_N -> PF_E_TOOLARGE. */
#define PF_CLUSTER_MAX_N 1024
#define PF_CLUSTER_GROMOS 0
#define PF_CLUSTER_SINGLE 1
#define PF_CLUSTER_COMPLETE 2
#define PF_CLUSTER_AVERAGE 3
typedef struct {
    const float* dist;                                              /* [B,B] */
    const int* index;                                               /* [B] */
    const int* offsets;                                             /* [G+1] */
    const float* score;                                             /* [B] optional */
    void* work;                                                     /* G x pf_cluster_work_bytes(n_max, method) bytes */
    int* label; int* cluster_size; int* representative;             /* [B] */
    int* best;                                                      /* [B], with score */
    int* n_neighbours;                                              /* [B] */
    int* n_clusters;                                                /* [G] */
    int B, G, n_max, method;
    float cutoff;                                                   /* >= 0 */
} pf_cluster_args;
int pf_cluster_fwd(const pf_cluster_args* a, pf_stream_t stream);
int pf_cluster_work_bytes(int n_max, int method);  /* scratch bytes per group (-1 for n_max outside [1, PF_CLUSTER_MAX_N] or a bad method) */

/* ---- rotamer side-chain packing (ABI 65, added entry points) -----------------------------------------------------------------------
 * pf_pack_sidechains_fwd: every rotamer of a discrete table built on the backbone of each movable residue, scored against the fixed
 * environment and against each other with the pair function of pf_interface_energy_fwd, and one chosen per residue by iterated
 * conditional modes; the conventions are listed in csrc/packing.hip.  It is NOT SCWRL4 and NOT Rosetta's packer (no Dunbrack library,
 * no hydrogens, no fitted parameter; a local search): it takes their place in role only.  Inputs as pf_relax_fwd; a movable residue
 * of a type in 0..19 with N, CA and C is packed, every other residue is fixed environment and is copied bit for bit.
 *   pos_out [B,N,15,3], mask_out [B,N,15]; packed [B,N]; rotamer [B,N] (-1: not packed); chi [B,N,4]; n_rotamers [B,N];
 *   energy_self_best [B,N] (E_self of the start); energy_residue [B,N] (E_self + half the pair terms at the end);
 *   energy_trace [B,sweeps+1] float64 ([0]: the start; sweeps not run repeat the last); sweeps_run [B]; changed [B,sweeps];
 *   choice_trace [B,sweeps,N] optional: the rotamer taken at each visit (entries not visited are left as they are).
 * work: pf_pack_work_bytes(B, N, max_rot) bytes, 16-byte aligned, no initialisation needed (-1: N > PF_PACK_MAX_N, max_rot outside
 * 1 .. PF_PACK_MAX_ROT, a negative size, or more than INT_MAX bytes).  Three launches, no atomics, one writer per output, every sum in
 * a fixed order, every decision an argmin under (value, index): bit-identical from run to run and independent of the rest of the
 * batch; the host reads nothing back.  N > PF_PACK_MAX_N, max_rot > PF_PACK_MAX_ROT or B > 65535 -> PF_E_TOOLARGE. */
#define PF_PACK_MAX_N 512
#define PF_PACK_MAX_ROT 128
#define PF_PACK_SLOTS 15
#define PF_PACK_ROT_ATOMS 9
typedef struct {
    const float* pos;                                               /* [B,N,n_atoms,3] */
    const unsigned char* atom_mask;                                 /* [B,N,n_atoms] */
    const int64_t* aa;                                              /* [B,N] */
    const int* residue_index;                                       /* [B,N] */
    const unsigned char* movable;                                   /* [B,N] */
    const float* radius;                                            /* [21,15] XS radii, 0: the type has no such atom */
    const unsigned char* types;                                     /* [21,15] bit 0 hydrophobic, bit 1 donor, bit 2 acceptor */
    const int* own_mask;                                            /* [21,15] bit b of (t, a): own-residue pair (a, b) is evaluated */
    const float* tab_rot;                                           /* [21,8,9] the rigid groups' rotations */
    const float* tab_trans;                                         /* [21,8,3] and translations */
    const int* tab_group;                                           /* [21,14] rigid group of each slot */
    const float* tab_pos;                                           /* [21,14,3] ideal position in its group's frame */
    const unsigned char* tab_mask;                                  /* [22,15] the type's heavy atoms */
    const float* rot_chi;                                           /* [21,max_rot,4] radians */
    const int* rot_count;                                           /* [21] */
    const float* rot_energy;                                        /* [21,max_rot] */
    void* work;                                                     /* pf_pack_work_bytes(B, N, max_rot) bytes */
    float* pos_out;                                                 /* [B,N,15,3] */
    unsigned char* mask_out;                                        /* [B,N,15] */
    unsigned char* packed;                                          /* [B,N] */
    int* rotamer;                                                   /* [B,N] */
    float* chi;                                                     /* [B,N,4] */
    int* n_rotamers;                                                /* [B,N] */
    float* energy_self_best;                                        /* [B,N] */
    float* energy_residue;                                          /* [B,N] */
    double* energy_trace;                                           /* [B,sweeps+1] */
    int* sweeps_run;                                                /* [B] */
    int* changed;                                                   /* [B,sweeps]; may be null when sweeps is 0 */
    int* choice_trace;                                              /* [B,sweeps,N] optional */
    int B, N, n_atoms, max_rot, sweeps, pro, cys;
    float cutoff;                                                   /* > 0; 8.0 */
    float w_gauss1, w_gauss2, w_repulsion, w_hydrophobic, w_hbond;  /* -0.0356, -0.00516, 0.840, -0.0351, -0.587 */
} pf_pack_args;
int pf_pack_sidechains_fwd(const pf_pack_args* a, pf_stream_t stream);
int pf_pack_work_bytes(int B, int N, int max_rot);

/* ---- point-mutation scanning (ABI 65, added entry points) --------------------------------------------------------------------------
 * pf_mutation_scan_fwd: at every scanned residue (positions set, type in 0..19, N, CA and C present) every rotamer of each candidate
 * residue type is built on the residue's own backbone and scored as pf_pack_sidechains_fwd scores E_self -- against every other residue
 * exactly as given (side chains included; neighbours are not repacked), its own residue with the fixed atoms, radii, type bits and
 * own_mask of the CANDIDATE type, plus rot_energy -- and the best rotamer per type is reported; the conventions are listed in
 * csrc/mutscan.hip.  energy[q,t] - energy[q,aa[q]] is what an alanine scan (t = ALA) or a position scan reports.  It is NOT FoldX and
 * NOT Rosetta (no solvation, electrostatics, entropy or backbone movement; untuned): it takes their place in role only.  Tables,
 * rotamer table, cutoff, weights, pro and cys as pf_pack_args; candidates [B,N,20] optional (null: all; the wild type is always
 * evaluated); group [B,N] optional.
 *   scanned [B,N]; energy [B,N,20] (+inf where not evaluated) with the bits of pf_pack_sidechains_fwd's energy_self_best on the input
 *   with aa[q] := t and q alone movable; rotamer [B,N,20] (-1); n_rotamers [B,N,20] (0); chi [B,N,20,4] (the chosen row; 0);
 *   energy_interface [B,N,20] (+inf): the chosen rotamer's terms against residues of another group byte (0 without group).
 * work: pf_mutation_scan_work_bytes(B, N) bytes (272 per residue: nothing per type or rotamer), 16-byte aligned, no initialisation
 * needed (-1: N > PF_PACK_MAX_N, a negative size, or more than INT_MAX bytes).  Two launches, no atomics, one writer per output, every
 * sum in packing's order: bit-identical from run to run and independent of the rest of the batch, of the other positions and of the
 * other candidates; the host reads nothing back.  N > PF_PACK_MAX_N, max_rot > PF_PACK_MAX_ROT or B > 65535 -> PF_E_TOOLARGE. */
#define PF_MUTATION_SCAN_TYPES 20
typedef struct {
    const float* pos;                                               /* [B,N,n_atoms,3] */
    const unsigned char* atom_mask;                                 /* [B,N,n_atoms] */
    const int64_t* aa;                                              /* [B,N] */
    const int* residue_index;                                       /* [B,N] */
    const unsigned char* positions;                                 /* [B,N] */
    const unsigned char* candidates;                                /* [B,N,20] optional */
    const unsigned char* group;                                     /* [B,N] optional */
    const float* radius;                                            /* [21,15] as pf_pack_args, down to rot_energy */
    const unsigned char* types;                                     /* [21,15] */
    const int* own_mask;                                            /* [21,15] */
    const float* tab_rot;                                           /* [21,8,9] */
    const float* tab_trans;                                         /* [21,8,3] */
    const int* tab_group;                                           /* [21,14] */
    const float* tab_pos;                                           /* [21,14,3] */
    const unsigned char* tab_mask;                                  /* [22,15] */
    const float* rot_chi;                                           /* [21,max_rot,4] radians */
    const int* rot_count;                                           /* [21] */
    const float* rot_energy;                                        /* [21,max_rot] */
    void* work;                                                     /* pf_mutation_scan_work_bytes(B, N) bytes */
    unsigned char* scanned;                                         /* [B,N] */
    float* energy;                                                  /* [B,N,20] */
    int* rotamer;                                                   /* [B,N,20] */
    int* n_rotamers;                                                /* [B,N,20] */
    float* chi;                                                     /* [B,N,20,4] */
    float* energy_interface;                                        /* [B,N,20] */
    int B, N, n_atoms, max_rot, pro, cys;
    float cutoff;                                                   /* > 0; 8.0 */
    float w_gauss1, w_gauss2, w_repulsion, w_hydrophobic, w_hbond;  /* -0.0356, -0.00516, 0.840, -0.0351, -0.587 */
} pf_mutation_scan_args;
int pf_mutation_scan_fwd(const pf_mutation_scan_args* a, pf_stream_t stream);
int pf_mutation_scan_work_bytes(int B, int N);

/* ---- fixed-backbone sequence design (ABI 65, added entry points) --------------------------------------------------------------------
 * pf_sequence_design_fwd: residue TYPE and rotamer of the designed residues of each structure are chosen together, on the fixed
 * backbone, by iterated conditional modes over every candidate (type, rotamer): pf_mutation_scan_fwd's E_self of every candidate
 * against the residues that are not designed, plus the pair terms between the designed residues, whose CB, radii and type bits follow
 * their current type; the conventions are listed in csrc/seqdesign.hip.  It stands where the reference's eval/run_mpnn.py runs
 * ProteinMPNN over backbone-only samples, in role only: it is NOT ProteinMPNN and NOT Rosetta fixbb.  The energy is this package's
 * Vina-form pair energy plus the rotamer table's energy plus the caller's per-type reference energy: no solvation, no electrostatics,
 * no entropy, no learned prior; without reference energies it favours large side chains; a deterministic local search; untuned.
 * Tables, rotamer table, cutoff, weights, pro, cys and sweeps as pf_pack_args.  A residue is designed where `designed` is set, its type
 * is in 0..19 and its N, CA and C are present; its candidates are the types whose byte is set (null: all 20; none set: its own type).
 * A sample with more than max_res (<= PF_SEQ_DESIGN_MAX_RES) such residues gets status 1 and comes back as if none were designed.
 *   aa_out [B,N]; pos_out [B,N,15,3], mask_out [B,N,15] as pf_pack_sidechains_fwd; designed_out [B,N]; status [B]; rotamer [B,N] (-1);
 *   chi [B,N,4]; n_candidates [B,N] (0); energy_self_best [B,N] (E_self of the start); energy_residue [B,N] (E_self + half the pair
 *   terms at the end); energy_trace [B,sweeps+1] float64; sweeps_run [B]; changed, changed_types [B,sweeps]; profile [B,N,20] (the
 *   smallest conditional energy of each candidate type against the final state of the others; +inf), profile_rotamer [B,N,20] (-1);
 *   choice_trace [B,sweeps,N,2] optional: type and rotamer taken at each visit (entries not visited are left as they are).
 * work: pf_sequence_design_work_bytes(B, N, max_rot, max_res) bytes = B (16 + 276 N + max_res (4 + 80 + 80 max_rot)), 16-byte aligned,
 * no initialisation needed (-1: N > PF_PACK_MAX_N, max_rot or max_res out of range, a negative size, or more than INT_MAX bytes).
 * Three launches, no atomics, one writer per output, every sum in a fixed order, every decision an argmin under (value, type,
 * rotamer): bit-identical from run to run and independent of the rest of the batch; the host reads nothing back. */
#define PF_SEQ_DESIGN_MAX_RES 64
#define PF_SEQ_DESIGN_TYPES 20
typedef struct {
    const float* pos;                                               /* [B,N,n_atoms,3] */
    const unsigned char* atom_mask;                                 /* [B,N,n_atoms] */
    const int64_t* aa;                                              /* [B,N] */
    const int* residue_index;                                       /* [B,N] */
    const unsigned char* designed;                                  /* [B,N] */
    const unsigned char* candidates;                                /* [B,N,20] optional */
    const float* ref_energy;                                        /* [20] optional */
    const float* radius;                                            /* [21,15] as pf_pack_args, down to rot_energy */
    const unsigned char* types;                                     /* [21,15] */
    const int* own_mask;                                            /* [21,15] */
    const float* tab_rot;                                           /* [21,8,9] */
    const float* tab_trans;                                         /* [21,8,3] */
    const int* tab_group;                                           /* [21,14] */
    const float* tab_pos;                                           /* [21,14,3] */
    const unsigned char* tab_mask;                                  /* [22,15] */
    const float* rot_chi;                                           /* [21,max_rot,4] radians */
    const int* rot_count;                                           /* [21] */
    const float* rot_energy;                                        /* [21,max_rot] */
    void* work;                                                     /* pf_sequence_design_work_bytes(B, N, max_rot, max_res) bytes */
    int64_t* aa_out;                                                /* [B,N] */
    float* pos_out;                                                 /* [B,N,15,3] */
    unsigned char* mask_out;                                        /* [B,N,15] */
    unsigned char* designed_out;                                    /* [B,N] */
    int* status;                                                    /* [B] */
    int* rotamer;                                                   /* [B,N] */
    float* chi;                                                     /* [B,N,4] */
    int* n_candidates;                                              /* [B,N] */
    float* energy_self_best;                                        /* [B,N] */
    float* energy_residue;                                          /* [B,N] */
    double* energy_trace;                                           /* [B,sweeps+1] */
    int* sweeps_run;                                                /* [B] */
    int* changed;                                                   /* [B,sweeps]; may be null when sweeps is 0 */
    int* changed_types;                                             /* [B,sweeps]; may be null when sweeps is 0 */
    float* profile;                                                 /* [B,N,20] */
    int* profile_rotamer;                                           /* [B,N,20] */
    int* choice_trace;                                              /* [B,sweeps,N,2] optional */
    int B, N, n_atoms, max_rot, max_res, sweeps, pro, cys;
    float cutoff;                                                   /* > 0; 8.0 */
    float w_gauss1, w_gauss2, w_repulsion, w_hydrophobic, w_hbond;  /* -0.0356, -0.00516, 0.840, -0.0351, -0.587 */
} pf_sequence_design_args;
int pf_sequence_design_fwd(const pf_sequence_design_args* a, pf_stream_t stream);
int pf_sequence_design_work_bytes(int B, int N, int max_rot, int max_res);

/* ---- empirical interface energy (ABI 64, added entry point) -----------------------------------------------------------------------
 * pf_interface_energy_fwd: the functional form of AutoDock Vina's scoring function (Trott & Olson, J. Comput. Chem. 2010) over the
 * heavy atoms of a batch of structures, between atoms of residues whose group bytes differ; the conventions are listed in
 * csrc/interface_energy.hip.  Written from the publication and checked against a float64 restatement; it is not checked against the
 * Vina program, and it is neither Vina's output nor Rosetta's dG_separated.  Slots 0 .. min(n_atoms, 15) - 1 are read; an atom takes
 * part where atom_mask is set and radius has an entry for its type and slot.  A pair counts when r < cutoff; d = r - R_i - R_j.
 *   terms_atom [B,N,15,5]        per row atom, the unweighted sums of gauss1, gauss2, repulsion, hydrophobic, hbond over its partners;
 *   pairs_atom, hbond_pairs_atom, hydrophobic_pairs_atom [B,N,15]   partners inside the cutoff, with hbond > 0, with hydrophobic > 0;
 *   terms_residue [B,N,5]        the sum over the slots;  energy_residue [B,N] = sum_k w_k terms_residue[k].
 * Each pair shows in both of its rows.  With query only atoms of query residues are rows (a participating atom that is not one has
 * counts -1 and zero terms); every participating atom is still a partner.  work: [B,N,4] floats, no initialisation needed.  Two
 * launches, no atomics, nothing pair-sized, one writer per output: bit-identical from run to run and independent of the rest of the
 * batch.  N > PF_INTERFACE_ENERGY_MAX_N or B > 65535 -> PF_E_TOOLARGE. */
#define PF_INTERFACE_ENERGY_MAX_N 512
#define PF_INTERFACE_ENERGY_SLOTS 15
typedef struct {
    const float* pos;                                               /* [B,N,n_atoms,3] */
    const unsigned char* atom_mask;                                 /* [B,N,n_atoms] */
    const int64_t* aa;                                              /* [B,N] */
    const unsigned char* group;                                     /* [B,N] */
    const unsigned char* query;                                     /* [B,N] optional */
    const float* radius;                                            /* [21,15] XS radii, 0: the type has no such atom */
    const unsigned char* types;                                     /* [21,15] bit 0 hydrophobic, bit 1 donor, bit 2 acceptor */
    float* work;                                                    /* [B,N,4] */
    float* terms_atom;                                              /* [B,N,15,5] */
    float* terms_residue;                                           /* [B,N,5] */
    float* energy_residue;                                          /* [B,N] */
    int* pairs_atom; int* hbond_pairs_atom; int* hydrophobic_pairs_atom;    /* [B,N,15] */
    int B, N, n_atoms;
    float cutoff;                                                   /* > 0; 8.0 */
    float w_gauss1, w_gauss2, w_repulsion, w_hydrophobic, w_hbond;  /* -0.0356, -0.00516, 0.840, -0.0351, -0.587 */
} pf_interface_energy_args;
int pf_interface_energy_fwd(const pf_interface_energy_args* a, pf_stream_t stream);

/* ---- restrained relaxation (ABI 64, added entry points) ---------------------------------------------------------------------------
 * A restraint force field over the heavy atoms of a batch of structures and a monotone steepest-descent minimiser around it; the
 * conventions are listed in csrc/relax.hip.  It is NOT Amber and NOT Rosetta: E = E_rest + E_intra + E_conn + E_clash is built from
 * the clash overlap and the peptide-bond ideals of pf_violations_fwd and from the reference structure's own internal distances.
 * Slots 0 .. min(n_atoms, 15) - 1 are read; an atom exists where atom_mask is set and radius has an entry for its type and slot; the
 * existing atoms of movable residues move, every other atom is a fixed partner.
 *   pf_relax_energy_fwd   one evaluation at pos: gradient [B,N,15,3] (zero on atoms that do not move), terms_atom [B,N,15,4] (rest,
 *                         intra, conn, clash: every pair and connection counted once over the atoms), energy_atom [B,N,15] (optional),
 *                         terms [B,4] and energy [B] (float64 sums in a fixed order).  Reads nothing below `energy`.
 *   pf_relax_fwd          `steps` iterations from pos: trial y = x - alpha g on the moving atoms, accepted when E(y) <= E(x) in the
 *                         float64 sums (alpha *= 1.2), else rejected (alpha *= 0.5); a sample whose max|g| <= gtol is frozen.  x, g, y
 *                         [B,N,15,3] are the state (x: the result; atoms that do not move are copies of pos); gradient / terms_atom
 *                         are the trial's; terms / energy the accepted state's; terms_initial [B,4]; energy_trace [B,steps+1];
 *                         accepted [B,steps]; step_size [B,steps]; alpha, grad_max [B]; frozen, iterations [B].  1 + 2 (steps + 1)
 *                         launches, no host readback.
 * work: [B,N,4] floats, no initialisation needed.  No atomics, nothing pair-sized, one writer per output and every sum in a fixed
 * order: bit-identical from run to run and independent of the rest of the batch.  N > PF_RELAX_MAX_N or B > 65535 -> PF_E_TOOLARGE. */
#define PF_RELAX_MAX_N 512
#define PF_RELAX_SLOTS 15
#define PF_RELAX_TERMS 4
typedef struct {
    const float* pos;                                               /* [B,N,n_atoms,3] */
    const float* ref_pos;                                           /* [B,N,n_atoms,3] the restraint and internal-geometry reference */
    const unsigned char* atom_mask;                                 /* [B,N,n_atoms] */
    const int64_t* aa;                                              /* [B,N] */
    const int* residue_index;                                       /* [B,N] */
    const unsigned char* movable;                                   /* [B,N] */
    const float* radius;                                            /* [21,15] van der Waals radii, 0: the type has no such atom */
    const int* pair_mask;                                           /* [21,15] bit b of (t, a): slots a and b of type t are restrained */
    float* work;                                                    /* [B,N,4] */
    float* gradient;                                                /* [B,N,15,3] */
    float* terms_atom;                                              /* [B,N,15,4] */
    float* energy_atom;                                             /* [B,N,15] optional */
    double* terms;                                                  /* [B,4] */
    double* energy;                                                 /* [B] */
    float* x; float* g; float* y;                                   /* [B,N,15,3] pf_relax_fwd: accepted positions, gradient; trial */
    float* alpha;                                                   /* [B] */
    int* frozen;                                                    /* [B] */
    double* terms_initial;                                          /* [B,4] */
    double* energy_trace;                                           /* [B,steps+1] */
    unsigned char* accepted;                                        /* [B,steps] */
    float* step_size;                                               /* [B,steps] */
    float* grad_max;                                                /* [B] */
    int* iterations;                                                /* [B] */
    int B, N, n_atoms, pro, steps;
    float k_rest, k_intra, k_bond, k_angle, k_clash;                /* > 0; 10, 300, 300, 150, 200 */
    float clash_overlap_tolerance, clash_margin;                    /* 1.5, 0.2 */
    float step0, gtol;                                              /* > 0, >= 0; 0.002, 0 */
} pf_relax_args;
int pf_relax_energy_fwd(const pf_relax_args* a, pf_stream_t stream);
int pf_relax_fwd(const pf_relax_args* a, pf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
