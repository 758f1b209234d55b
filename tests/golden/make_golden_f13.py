"""F13: the reference's `align` / `batch_align` (pepflow/modules/common/geometry.py:18-56: r = V U^T from the SVD of S = X^T Y over the
masked atoms, no determinant correction, applied with its translation to every atom) on seeded inputs: coordinates up to +-50 A,
masked atoms, equal per-sample mask counts in the batched case, and one mirror-image pair whose rotation has det = -1.
Build container only (needs the reference).  Data only.  Re-run: python tests/golden/make_golden_f13.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "tools"))
import ref_shim  # noqa: E402
ref_shim.build_reference_model()
from pepflow.modules.common import geometry as G  # noqa: E402

g = torch.Generator().manual_seed(1301)


def rand_rot():
    q = torch.randn(4, generator=g, dtype=torch.float64)
    a, b, c, d = (q / q.norm()).tolist()
    return torch.tensor([[a*a+b*b-c*c-d*d, 2*(b*c-a*d), 2*(b*d+a*c)], [2*(b*c+a*d), a*a-b*b+c*c-d*d, 2*(c*d-a*b)],
                         [2*(b*d-a*c), 2*(c*d+a*b), a*a-b*b-c*c+d*d]], dtype=torch.float64)


def moved(x, noise):
    """a rigidly moved, noisy copy of x [..., 3] (float64 in, float32 out)"""
    y = x @ rand_rot().T + (torch.rand(3, generator=g, dtype=torch.float64) * 40 - 20) + noise * torch.randn(x.shape, generator=g, dtype=torch.float64)
    return y.float()


def fit_det(p1, aligned):
    """det of the rotation the reference applied (least squares over all atoms: aligned = r p1 + t)"""
    a, b = p1.reshape(-1, 3).double(), aligned.reshape(-1, 3).double()
    a, b = a - a.mean(0), b - b.mean(0)
    r = torch.linalg.lstsq(a, b).solution.T
    return float(torch.linalg.det(r))


out = {}
# single complex: L = 12 residues x A = 4 atoms, +-50 A, ~20 % of the atoms masked
L, A = 12, 4
x = (torch.rand(L, A, 3, generator=g, dtype=torch.float64) * 100 - 50)
m = torch.rand(L, A, generator=g) > 0.2
p1, p2 = x.float(), moved(x, 1.5)
a1, _ = G.align(p1, p2, m)
out.update(align_pos_1=p1.numpy(), align_pos_2=p2.numpy(), align_mask=m.numpy(), align_out=a1.numpy())

# mirror image: pos_2 is a reflected, moved, slightly noisy copy -> the reference's rotation is a reflection (det = -1)
x = (torch.rand(L, A, 3, generator=g, dtype=torch.float64) * 60 - 30)
m = torch.rand(L, A, generator=g) > 0.2
p1 = x.float()
p2 = moved(x * torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64), 0.05)
a1, _ = G.align(p1, p2, m)
out.update(mirror_pos_1=p1.numpy(), mirror_pos_2=p2.numpy(), mirror_mask=m.numpy(), mirror_out=a1.numpy(), mirror_det=fit_det(p1, a1))

# batch: B = 5 samples of L = 10 x A = 5, the same number of atoms masked in every sample (at different places)
B, L, A = 5, 10, 5
x = (torch.rand(B, L, A, 3, generator=g, dtype=torch.float64) * 100 - 50)
m = torch.ones(B, L * A, dtype=torch.bool)
for b in range(B):
    m[b, torch.randperm(L * A, generator=g)[:9]] = False
m = m.reshape(B, L, A)
p1 = x.float()
p2 = torch.stack([moved(x[b], 2.0) for b in range(B)])
a1, _ = G.batch_align(p1, p2, m)
out.update(batch_pos_1=p1.numpy(), batch_pos_2=p2.numpy(), batch_mask=m.numpy(), batch_out=a1.numpy())

np.savez_compressed(os.path.join(HERE, "f13_align.npz"), **out)
print("f13:", {k: v.shape for k, v in out.items() if hasattr(v, "shape")}, "mirror det", out["mirror_det"])
