"""The keys of the fp32 IPA score kernel as ONE fragment buffer per sample (pf_ipa_attn_args.k_frag_s; csrc/common.h
pf_kfrag_put), written by the kernels that produce the node state (pf_input_mixer_fwd, the last pf_node_tfmr_fwd of a block) and read
by the eight head workgroups of the sample, at the smallest shapes where the layout can go wrong (`pytest -m gpu`):

  (2, 80)   key ends (67, 6)   a partial last tile; a sample shorter than one tile
  (2, 128)  dense              the shape of the flagship workload
  (1, 96)   dense              an odd number of 32-key steps
  (40, 112) ragged             more 16-row tiles than CUs: the 32-row form of node_tfmr, whose last tile is half empty (7 tiles)

The form for L <= 64 (fp32 fragments, the score kernel with the pair phase) keeps its per-head fragments: nothing of it is shared, so
no (2, 48) case here."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pepflow_oracle as O  # noqa: E402  (checker only)
from pepflowww_amd import synth, _capi  # noqa: E402
from pepflowww_amd.engine import DenoiseEngine, PackedWeights  # noqa: E402
import gpu_util as G  # noqa: E402

SHAPES = [(2, 80, (67, 6)), (2, 128, None), (1, 96, None), (40, 112, tuple(112 - (5 * i) % 100 for i in range(40)))]
_IDS = [f"{b}x{l}" + ("" if ke is None else "-ragged") for b, l, ke in SHAPES]


def cu(t):
    return t.to(G.dev()).contiguous()


def expected_fragments(s, L):
    """The layout, stated once more in numpy.  s: [B, L, 128] float32 -> [B, tiles, 4096] float16: per 16-key tile 8 KiB; 32-channel
    K-step st = 2 KiB = hi KiB then lo KiB; in a KiB lane (key r, g) holds 16 bytes: halves 0..3 = channels 32 st + 4 g .. + 3,
    halves 4..7 = channels 32 st + 16 + 4 g .. + 3.  hi = float16(v), lo = float16(v - float32(hi))."""
    B = s.shape[0]
    tiles = (L + 15) // 16
    v = np.zeros((B, tiles * 16, 128), np.float32)
    v[:, :L] = s
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    out = np.zeros((B, tiles, 4096), np.float16)
    i, c = np.meshgrid(np.arange(tiles * 16), np.arange(128), indexing="ij")
    tile, r = i // 16, i % 16
    st, slot, g, e = c // 32, (c % 32) // 16, (c % 16) // 4, c % 4
    for plane, src in ((0, hi), (1, lo)):
        idx = st * 1024 + plane * 512 + (r + 16 * g) * 8 + slot * 4 + e
        out[:, tile, idx] = src[:, i, c]
    return out


def _rows_below_key_end(L, kend):
    """Boolean [B, tiles, 4096]: the halves of the buffer that belong to rows below each sample's key end."""
    tiles = (L + 15) // 16
    row = np.zeros((tiles, 4096), np.int64)
    lane = (np.arange(4096) % 512) // 8
    row[:] = (lane % 16)[None, :]
    row += 16 * np.arange(tiles)[:, None]
    return row[None] < np.asarray(kend)[:, None, None]


def _engine(seeded_sd, B, L, kend, seed):
    """An engine on a random context (the fragment tests need no oracle), its key ends, and the step's state set."""
    w = PackedWeights({k: cu(v) for k, v in seeded_sd.items()}, G.dev())
    g = torch.Generator().manual_seed(seed)
    kend = [L] * B if kend is None else list(kend)
    mask = torch.arange(L)[None, :] < torch.tensor(kend)[:, None]
    eng = DenoiseEngine(w, B, L, G.dev(), precision="fp32")
    assert eng.fused_proj and eng.k_fold and not eng.fused_pair and eng.k_frag_s is not None
    eng.bind_context(cu(torch.randn(B, L, 128, generator=g)), cu(torch.randn(B, L, L, 64, generator=g)), cu(mask))
    q = torch.randn(B, L, 4, generator=g)
    eng.set_state(cu(torch.rand(B, 1, generator=g) * 0.9 + 0.05), cu(O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))),
                  cu(torch.randn(B, L, 3, generator=g) * 8), cu(torch.rand(B, L, 5, generator=g) * 2 * math.pi), cu(torch.randint(0, 20, (B, L), generator=g)))
    return eng, kend


def _launch(entry):
    fn, args, name = entry[0], entry[1], entry[2]
    _capi.check(fn(args, _capi.stream_ptr()), name)


def _check_fragments(eng, kend, what):
    G.sync()
    B, L = eng.B, eng.L
    got = eng.k_frag_s.cpu().numpy().reshape(B, -1, 4096)
    want = expected_fragments(eng.s.cpu().numpy().reshape(B, L, 128), L)
    live = _rows_below_key_end(L, kend)
    assert np.isfinite(got.astype(np.float32)).all(), what
    assert np.array_equal(got.view(np.uint16)[live], want.view(np.uint16)[live]), what


@pytest.fixture(scope="module", params=SHAPES, ids=_IDS)
def block1(request, seeded_sd):
    """One step of the plan, launch by launch, up to block 1's attention: the producers' fragments are checked on the way (test 1 of
    the three below runs here, once per shape); what the tests share is the engine stopped in front of that attention call."""
    B, L, ke = request.param
    eng, kend = _engine(seeded_sd, B, L, ke, 4100 + L)
    checked, n_attn, ia = [], 0, None
    for entry in eng.plan:
        if entry[0] is None:
            continue
        obj = entry[1]._obj
        if entry[2] == "pf_ipa_attn_fwd":
            n_attn += 1
            if n_attn == 2:
                ia = obj
                break
        _launch(entry)
        if entry[2] == "pf_input_mixer_fwd" or (entry[2] == "pf_node_tfmr_fwd" and obj.last):
            assert obj.k_frag_s == eng.k_frag_s.data_ptr()
            _check_fragments(eng, kend, entry[2])
            checked.append(entry[2])
    assert checked == ["pf_input_mixer_fwd", "pf_node_tfmr_fwd"] and ia is not None
    if B * ((L + 15) // 16) > 256:
        assert B * ((L + 31) // 32) <= 256                 # (the 32-row form of node_tfmr ran, in one round)
    return eng, kend, ia


def _attend(eng, ia):
    eng.feats.fill_(float("nan"))
    eng.attn_p.fill_(float("nan"))
    _capi.check(_capi.load().pf_ipa_attn_fwd(C.byref(ia), _capi.stream_ptr()), "pf_ipa_attn_fwd")
    G.sync()
    return eng.feats.clone().view(torch.int32), eng.attn_p.clone().view(torch.int32)


def test_producers_write_the_fragments_of_their_rows(block1):
    """Test 1: what pf_input_mixer_fwd and the block's last pf_node_tfmr_fwd wrote into the shared buffer is, byte for byte, the numpy
    statement of the layout applied to the node state the same launch stored, over all rows below each sample's key end (asserted
    while the fixture walks the plan; here: the buffer still equals block 0's output in front of block 1's attention)."""
    eng, kend, _ = block1
    _check_fragments(eng, kend, "in front of block 1's attention")


def test_attention_with_shared_and_with_its_own_fragments(block1):
    """Test 2: pf_ipa_attn_fwd with the producer-written buffer and with the pointer NULL (the stand-alone path: ipa_kfrag_kernel
    in front) -- every output identical, and each identical run to run."""
    eng, kend, ia = block1
    shared = ia.k_frag_s
    assert shared == eng.k_frag_s.data_ptr()
    try:
        a1, a2 = _attend(eng, ia), _attend(eng, ia)
        ia.k_frag_s = None
        b1, b2 = _attend(eng, ia), _attend(eng, ia)
    finally:
        ia.k_frag_s = shared
    for x, y in ((a1, a2), (b1, b2), (a1, b1)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    live = cu(torch.arange(eng.L)[None, :] < torch.tensor(kend)[:, None]).reshape(-1)
    assert torch.isfinite(a1[0].view(torch.float32)[live]).all()


def test_rows_beyond_the_key_end_reach_nothing(block1):
    """Test 4: the rows of a partial last tile at and beyond the key end hold the largest finite f16 value in both planes: the outputs
    are the bytes of the run without the fill (those keys pass through the mask SELECT of the tail tile only)."""
    eng, kend, ia = block1
    B, L = eng.B, eng.L
    tiles = (L + 15) // 16
    dead = ~_rows_below_key_end(L, kend) & _rows_below_key_end(L, [16 * ((k + 15) // 16) for k in kend])
    if not dead.any():                                     # (a dense shape whose length is a multiple of 16: no such rows exist)
        assert all(k % 16 == 0 for k in kend)
        return
    clean = _attend(eng, ia)
    keep = eng.k_frag_s.clone()
    try:
        buf = eng.k_frag_s.view(B, tiles, 4096)
        buf[cu(torch.from_numpy(dead))] = 65504.0
        dirty = _attend(eng, ia)
    finally:
        eng.k_frag_s.copy_(keep)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])


@pytest.mark.parametrize("B,L,lengths", [(2, 80, [67, 6]), (2, 80, None), (2, 128, None), (2, 128, [128, 41]), (1, 96, None), (1, 96, [77])])
def test_step_against_the_oracle(seeded_sd, B, L, lengths):
    """Test 3: one engine step (shared fragments on: the default of this form) against the float oracle at the 1e-4 bound of the
    existing IPA / step tests, dense and with key ends."""
    w = PackedWeights({k: cu(v) for k, v in seeded_sd.items()}, G.dev())
    batch = synth.make_pocket_batch(B, L, 8, seed=61, lengths=lengths)
    g = torch.Generator().manual_seed(5)
    enc = O.encode(seeded_sd, batch)
    t = torch.rand(B, 1, generator=g) * 0.9 + 0.05
    q = torch.randn(B, L, 4, generator=g)
    R_t = O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))
    x_t = enc[1] + torch.randn(B, L, 3, generator=g)
    ang_t = torch.rand(B, L, 5, generator=g) * 2 * math.pi
    seq_t = torch.randint(0, 20, (B, L), generator=g)
    eng = DenoiseEngine(w, B, L, G.dev(), precision="fp32")
    assert eng.k_frag_s is not None
    eng.bind_context(cu(enc[4]), cu(enc[5]), cu(batch["res_mask"]))
    eng.set_state(cu(t), cu(R_t), cu(x_t), cu(ang_t), cu(seq_t))
    eng.run()
    G.sync()
    ok = batch["res_mask"].reshape(-1)
    with torch.no_grad():
        ref = O.ga_encoder(seeded_sd, t, R_t, x_t, ang_t, seq_t, enc[4], enc[5], batch["res_mask"].long())
    G.assert_close(eng.rot.cpu()[ok], ref[0].reshape(-1, 9)[ok], 1e-4, "rot vs oracle")
    G.assert_close(eng.trans.cpu()[ok], ref[1].reshape(-1, 3)[ok], 1e-4, "trans vs oracle")
