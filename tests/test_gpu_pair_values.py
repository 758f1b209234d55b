"""Pair aggregation on the pair values (ipa_pair_dz_kernel / ipa_pair_dz16_kernel) at the shapes where its code branches: the float4
and the scalar staging of P (L % 4), the number of 16-key groups a launch is built for (NG = 5, 8, 9) and the number a short sample
takes inside it (pair_dz_pick), a key end inside a group, a nearly empty sample.  Through the C ABI, against the run that reads z,
against the oracle, and twice for run-to-run identity (`pytest -m gpu`)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import pepflow_oracle as O  # noqa: E402  (checker only)
import gpu_util as G  # noqa: E402

REL = 1e-4


def cu(t):
    return t.to(G.dev()).contiguous()


def _masks(B, L):
    mask = torch.ones(B, L)
    if (B, L) == (2, 68):
        mask[0, 67:] = 0                   # key end 67: five key groups, the last one ends inside a float4
    elif (B, L) == (2, 70):
        mask[0, 41:] = 0                   # three of five groups
        mask[0, 7] = 0                     # a hole inside
    elif (B, L) == (2, 128):
        pass                               # sample 0 dense: all eight groups
    else:
        mask[0, 131:] = 0                  # (1, 144): nine groups, key end inside the last one
        mask[0, 60] = 0
    if B > 1:
        mask[1, :] = 0
        mask[1, 3:9] = 1                   # six unmasked residues: key end 9
    return mask


@pytest.mark.parametrize("B,L", [(2, 68), (2, 70), (2, 128), (1, 144)])
def test_pair_values_kernel_shapes(seeded_sd, B, L):
    g = torch.Generator().manual_seed(2000 + L)
    pfx = "ga_encoder.trunk.ipa_2."
    s = torch.randn(B, L, 128, generator=g)
    z = torch.randn(B, L, L, 64, generator=g)
    q = torch.randn(B, L, 4, generator=g)
    R = O.quat_to_rot(q / q.norm(dim=-1, keepdim=True))
    x = torch.randn(B, L, 3, generator=g) * 8
    mask = _masks(B, L)
    kend = (mask.to(torch.int32) * torch.arange(1, L + 1, dtype=torch.int32)).amax(-1)
    sd = seeded_sd
    gq = lambda k: cu(sd[pfx + k])
    wproj = torch.cat([sd[pfx + n + ".weight"] for n in ("linear_q", "linear_kv", "linear_q_points", "linear_kv_points")], 0)
    bproj = torch.cat([sd[pfx + n + ".bias"] for n in ("linear_q", "linear_kv", "linear_q_points", "linear_kv_points")], 0)
    proj = G.linear(cu(s.reshape(B * L, 128)), cu(wproj), cu(bproj))
    bias = cu((math.sqrt(1.0 / 3.0) * F.linear(z, sd[pfx + "linear_b.weight"], sd[pfx + "linear_b.bias"])).reshape(B, L, L, 8).permute(0, 3, 1, 2))
    dz = cu(F.linear(z, sd[pfx + "down_z.weight"]).contiguous())
    dz16 = dz.to(torch.float16)
    run = lambda zz, dd, ke: G.ipa_feats(proj, zz, cu(R.reshape(B * L, 9)), cu(x.reshape(B * L, 3)), cu(mask.reshape(-1)),
                                         gq("linear_b.weight"), gq("linear_b.bias"), gq("down_z.weight"), gq("down_z.bias"), gq("head_weights"),
                                         B, L, bias=bias, p_out=torch.zeros(B, 8, L, L, device=G.dev()), variant=2, key_end=ke, dz=dd)[0].cpu()
    valid = mask.reshape(-1).bool()
    ref = O.ipa(sd, pfx[:-1], s, z, R, x, mask)[1].reshape(B * L, -1)
    beyond = (torch.arange(L)[None, :] >= kend[:, None]).reshape(-1)
    for ke in (None, cu(kend)):
        from_z = run(cu(z), None, ke)
        from_dz, again = run(None, dz, ke), run(None, dz, ke)
        assert torch.equal(again[valid], from_dz[valid])                             # every row, run to run
        assert torch.equal(from_dz[valid][:, :1408], from_z[valid][:, :1408])        # everything but o_pair is the same code
        G.assert_close(from_dz[valid], from_z[valid], 1e-5, "pair values vs z")
        G.assert_close(from_dz[valid][:, 1408:], from_z[valid][:, 1408:], 1e-5, "o_pair from pair values vs from z")
        G.assert_close(from_dz[valid], ref[valid], REL, "pair values vs oracle")
        G.assert_close(from_dz[valid][:, 1408:], ref[valid][:, 1408:], REL, "o_pair vs oracle")
        from_16, again16 = run(None, dz16, ke), run(None, dz16, ke)
        assert torch.equal(again16[valid], from_16[valid])
        G.assert_close(from_16[valid], from_z[valid], 2e-3, "f16 pair values vs z")
        G.assert_close(from_16[valid][:, 1408:], from_z[valid][:, 1408:], 2e-3, "o_pair from f16 pair values vs from z")
        if ke is not None and beyond.any():
            assert torch.isnan(from_dz[beyond]).all() and torch.isnan(from_16[beyond]).all()   # rows beyond a key end are not written
