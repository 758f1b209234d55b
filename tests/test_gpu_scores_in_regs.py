"""The fp32 IPA score kernel without the pair phase (projection inside, keys = the node state; 64 < L <= 128, L % 4 == 0) keeps a
lane's scores in registers from the first product to the second: tile and step guards are nested, tiles beyond a sample's key end
are preset to the mask value.  The smallest shapes at which that can go wrong (`pytest -m gpu`):

  (2, 68)   key ends (68, 5)        five tiles with a 4-key partial tail; a sample with a single (partial) tile
  (2, 96)   key ends (96, 33)       six and three tiles: an odd count with a partial tail
  (3, 112)  key ends (112, 97, 16)  seven tiles, seven tiles with a 1-key tail, exactly one full tile
  (2, 128)  dense                   eight tiles: every guard taken

Per shape: feats and probabilities against the float oracle at the 1e-4 of the existing attention tests; every call twice, equal
bytes; the sample's key fragments from their producer and from the stand-alone path (NULL), equal bytes; shape A, shape B, shape A
again, equal bytes (nothing of a launch survives in LDS or in the scratch); one engine step against the oracle at 1e-4.  The only
bit-for-bit pairing the existing tests make for this form is shared against own fragments (tests/test_gpu_shared_keys.py): its
pairings with the projection launch and with the fp32-MFMA form are bounds (tests/test_gpu_round4.py), so none is repeated here."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import pepflow_oracle as O  # noqa: E402  (checker only)
from pepflowww_amd import synth, _capi  # noqa: E402
from pepflowww_amd.engine import DenoiseEngine, PackedWeights, pack_ipa_projection, fold_keys_into_queries  # noqa: E402
import gpu_util as G  # noqa: E402

SHAPES = [(2, 68, (68, 5)), (2, 96, (96, 33)), (3, 112, (112, 97, 16)), (2, 128, (128, 128))]
_IDS = [f"{b}x{l}" for b, l, _ in SHAPES]
PFX = "ga_encoder.trunk.ipa_1."


def cu(t):
    return t.to(G.dev()).contiguous()


def oracle_probs(sd, s, z, R, x, mask):
    """softmax of oracle.ipa (ipa_pytorch.py:389-433), which returns the features only: the same statements, [B,H,L,L]."""
    B, L, _ = s.shape
    H, Cc, PQ, PV = O.N_HEAD, O.C_HID, O.N_QP, O.N_VP
    pfx = PFX[:-1]
    q = O.lin(sd, pfx + ".linear_q", s).view(B, L, H, Cc)
    k = O.lin(sd, pfx + ".linear_kv", s).view(B, L, H, 2 * Cc)[..., :Cc]

    def points(name, n):
        p = torch.stack(O.lin(sd, pfx + name, s).split(n, dim=-1), dim=-1)
        return O.rot_apply(R[:, :, None], p) + x[:, :, None]

    qp = points(".linear_q_points", H * PQ).view(B, L, H, PQ, 3)
    kp = points(".linear_kv_points", H * (PQ + PV)).view(B, L, H, PQ + PV, 3)[..., :PQ, :]
    a = torch.einsum("bihc,bjhc->bhij", q, k) * math.sqrt(1.0 / (3 * Cc))
    a = a + math.sqrt(1.0 / 3) * O.lin(sd, pfx + ".linear_b", z).permute(0, 3, 1, 2)
    d2 = ((qp[:, :, None] - kp[:, None]) ** 2).sum(-1)
    gamma = F.softplus(sd[pfx + ".head_weights"]) * math.sqrt(1.0 / (3 * (PQ * 9.0 / 2)))
    a = a + ((d2 * gamma[:, None]).sum(-1) * (-0.5)).permute(0, 3, 1, 2)
    a = a + (O.IPA_INF * (mask[:, :, None] * mask[:, None, :] - 1))[:, None]
    return torch.softmax(a, dim=-1)


class Case:
    """Inputs of one shape on the device, the call, and the oracle's answer (computed once per shape)."""

    def __init__(self, sd, B, L, kend):
        self.B, self.L, self.kend = B, L, kend
        g = torch.Generator().manual_seed(900 + L)
        s = torch.randn(B, L, 128, generator=g)
        z = torch.randn(B, L, L, 64, generator=g)
        q = torch.randn(B, L, 4, generator=g)
        R = O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))
        x = torch.randn(B, L, 3, generator=g) * 8
        mask = (torch.arange(L)[None, :] < torch.tensor(kend)[:, None]).float()
        self.valid = mask.reshape(-1).bool()
        gq = lambda k: cu(sd[PFX + k])  # noqa: E731
        names = ("linear_q", "linear_kv", "linear_q_points", "linear_kv_points")
        wproj, bproj = fold_keys_into_queries(torch.cat([sd[PFX + n + ".weight"] for n in names], 0), torch.cat([sd[PFX + n + ".bias"] for n in names], 0))
        self.w16, self.bp = pack_ipa_projection(cu(wproj), cu(bproj))
        self.s, self.R, self.x, self.m = cu(s.reshape(B * L, 128)), cu(R.reshape(B * L, 9)), cu(x.reshape(B * L, 3)), cu(mask.reshape(-1))
        zd = cu(z)
        self.bias = (math.sqrt(1.0 / 3.0) * F.linear(zd, gq("linear_b.weight"), gq("linear_b.bias"))).reshape(B, L, L, 8).permute(0, 3, 1, 2).contiguous()
        self.dz = F.linear(zd, gq("down_z.weight")).contiguous()
        self.ke = cu(torch.tensor(kend, dtype=torch.int32))
        self.w = [gq(k) for k in ("linear_b.weight", "linear_b.bias", "down_z.weight", "down_z.bias", "head_weights")]
        with torch.no_grad():
            self.ref_feats = O.ipa(sd, PFX[:-1], s, z, R, x, mask)[1].reshape(B * L, -1)
            self.ref_p = oracle_probs(sd, s, z, R, x, mask)

    def run(self):
        """pf_ipa_attn_fwd in the form under test: projection inside, keys from the node state, probabilities out, pair values in."""
        B, L = self.B, self.L
        p = torch.full((B, 8, L, L), float("nan"), device=G.dev())
        feats = G.ipa_feats(torch.full((B * L, 3744), float("nan"), device=G.dev()), None, self.R, self.x, self.m, *self.w, B, L, bias=self.bias,
                            p_out=p, variant=2, key_end=self.ke, dz=self.dz, fused_pair=False, fused_proj=(self.s, self.w16, self.bp), k_from_s=True)[0]
        return feats, p


@pytest.fixture(scope="module")
def cases(seeded_sd):
    made = {}

    def get(i):
        if i not in made:
            made[i] = Case(seeded_sd, *SHAPES[i])
        return made[i]
    return get


def _live(c, feats, p):
    """What the call defines: feature rows below each sample's key end, probabilities of those rows over the keys below it."""
    B, L = c.B, c.L
    on = c.valid.reshape(B, L)
    pm = (on[:, None, :, None] & on[:, None, None, :]).expand(B, 8, L, L)
    return feats.cpu()[c.valid], torch.where(pm, p.cpu(), torch.zeros(()))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=_IDS)
def test_attention_against_the_oracle_and_itself(cases, i):
    c = cases(i)
    f1, p1 = c.run()
    f2, p2 = c.run()
    lf1, lp1 = _live(c, f1, p1)
    lf2, lp2 = _live(c, f2, p2)
    assert torch.equal(lf1.view(torch.int32), lf2.view(torch.int32)) and torch.equal(lp1.view(torch.int32), lp2.view(torch.int32))
    on = c.valid.reshape(c.B, c.L)
    pm = (on[:, None, :, None] & on[:, None, None, :]).expand_as(c.ref_p)
    G.assert_close(lf1, c.ref_feats[c.valid], 1e-4, "feats vs oracle")
    G.assert_close(lp1, torch.where(pm, c.ref_p, torch.zeros(())), 1e-4, "probabilities vs oracle")
    rows = lp1.sum(-1)[on[:, None, :].expand(c.B, 8, c.L)]
    assert (rows - 1).abs().max() < 1e-5


@pytest.mark.parametrize("ia,ib", [(0, 3), (3, 0), (1, 2), (2, 1)], ids=["68-128-68", "128-68-128", "96-112-96", "112-96-112"])
def test_nothing_of_a_launch_survives_into_the_next(cases, ia, ib):
    """Shape A, shape B, shape A again: both A results are the same bytes (stale LDS, stale scratch, a register preset that a
    shorter sample relies on)."""
    a, b = cases(ia), cases(ib)
    first = _live(a, *a.run())
    b.run()
    again = _live(a, *a.run())
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))


def _engine_at_block1(sd, B, L, kend, seed):
    """An engine on a random context, run launch by launch up to block 1's attention call (the sample's key fragments then come
    from the last pf_node_tfmr_fwd of block 0): the engine and that call's argument struct."""
    w = PackedWeights({k: cu(v) for k, v in sd.items()}, G.dev())
    g = torch.Generator().manual_seed(seed)
    mask = torch.arange(L)[None, :] < torch.tensor(kend)[:, None]
    eng = DenoiseEngine(w, B, L, G.dev(), precision="fp32")
    assert eng.fused_proj and eng.k_fold and not eng.fused_pair and eng.k_frag_s is not None
    eng.bind_context(cu(torch.randn(B, L, 128, generator=g)), cu(torch.randn(B, L, L, 64, generator=g)), cu(mask))
    q = torch.randn(B, L, 4, generator=g)
    eng.set_state(cu(torch.rand(B, 1, generator=g) * 0.9 + 0.05), cu(O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))),
                  cu(torch.randn(B, L, 3, generator=g) * 8), cu(torch.rand(B, L, 5, generator=g) * 2 * math.pi), cu(torch.randint(0, 20, (B, L), generator=g)))
    n_attn = 0
    for entry in eng.plan:
        if entry[0] is None:
            continue
        if entry[2] == "pf_ipa_attn_fwd":
            n_attn += 1
            if n_attn == 2:
                return eng, entry[1]._obj
        _capi.check(entry[0](entry[1], _capi.stream_ptr()), entry[2])
    raise AssertionError("no second attention call in the plan")


@pytest.mark.parametrize("B,L,kend", SHAPES, ids=_IDS)
def test_fragments_from_the_producer_and_from_the_stand_alone_path(seeded_sd, B, L, kend):
    eng, ia = _engine_at_block1(seeded_sd, B, L, kend, 4300 + L)
    live = cu(torch.arange(L)[None, :] < torch.tensor(kend)[:, None])

    def attend():
        eng.feats.fill_(float("nan"))
        eng.attn_p.fill_(float("nan"))
        _capi.check(_capi.load().pf_ipa_attn_fwd(C.byref(ia), _capi.stream_ptr()), "pf_ipa_attn_fwd")
        G.sync()
        pm = (live[:, None, :, None] & live[:, None, None, :]).expand(B, 8, L, L)
        p = torch.where(pm, eng.attn_p.view(B, 8, L, L), torch.zeros((), device=G.dev()))
        return eng.feats[live.reshape(-1)].clone().view(torch.int32), p.view(torch.int32)
    shared = ia.k_frag_s
    assert shared == eng.k_frag_s.data_ptr()
    try:
        a1, a2 = attend(), attend()
        ia.k_frag_s = None
        b1, b2 = attend(), attend()
    finally:
        ia.k_frag_s = shared
    for x, y in ((a1, a2), (b1, b2), (a1, b1)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    assert torch.isfinite(a1[0].view(torch.float32)).all() and torch.isfinite(a1[1].view(torch.float32)).all()


@pytest.mark.parametrize("B,L,kend", SHAPES, ids=_IDS)
def test_step_against_the_oracle(seeded_sd, B, L, kend):
    w = PackedWeights({k: cu(v) for k, v in seeded_sd.items()}, G.dev())
    batch = synth.make_pocket_batch(B, L, 8, seed=67, lengths=list(kend))
    g = torch.Generator().manual_seed(9)
    enc = O.encode(seeded_sd, batch)
    t = torch.rand(B, 1, generator=g) * 0.9 + 0.05
    q = torch.randn(B, L, 4, generator=g)
    R_t = O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))
    x_t = enc[1] + torch.randn(B, L, 3, generator=g)
    ang_t = torch.rand(B, L, 5, generator=g) * 2 * math.pi
    seq_t = torch.randint(0, 20, (B, L), generator=g)
    eng = DenoiseEngine(w, B, L, G.dev(), precision="fp32")
    assert eng.fused_proj and eng.k_fold and not eng.fused_pair and eng.k_frag_s is not None
    eng.bind_context(cu(enc[4]), cu(enc[5]), cu(batch["res_mask"]))
    eng.set_state(cu(t), cu(R_t), cu(x_t), cu(ang_t), cu(seq_t))
    eng.run()
    G.sync()
    ok = batch["res_mask"].reshape(-1)
    with torch.no_grad():
        ref = O.ga_encoder(seeded_sd, t, R_t, x_t, ang_t, seq_t, enc[4], enc[5], batch["res_mask"].long())
    G.assert_close(eng.rot.cpu()[ok], ref[0].reshape(-1, 9)[ok], 1e-4, "rot vs oracle")
    G.assert_close(eng.trans.cpu()[ok], ref[1].reshape(-1, 3)[ok], 1e-4, "trans vs oracle")
