"""Batch-sharded sampling over the GPUs of one node.

Samples are independent (no cross-sample op anywhere on the path), so rank r of W runs the
contiguous shard [r*B/W, (r+1)*B/W) with replicated weights and NO data-path collective.  RNG
streams are keyed by the GLOBAL sample index (pre-drawn initial noise is sliced from the global
draw; the in-kernel Philox counter carries first_sample + b), so the result does not depend on W.
ONE collective closes the run: an all-gather of the packed final state over RCCL/xGMI
(torch.distributed backend "nccl"; "gloo" in the CPU tests of the host logic).

The reference has no sharded sampler (inference.py:71-76 loops complexes serially on one device);
train_ddp.py:79,94 is the only collective code path there.
"""
import math

import torch
import torch.distributed as dist

STATE_KEYS = (("rotmats", 9), ("trans", 3), ("angles", 5), ("seqs_simplex", 20), ("seqs", 1))
PACK_WIDTH = sum(n for _, n in STATE_KEYS)          # 38 floats per residue


def shard_bounds(total, world, rank):
    """Contiguous shards; the first (total % world) ranks get one extra sample."""
    base, extra = divmod(total, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def shard_batch(batch, world, rank):
    """Slice a PaddingCollate batch (pepflow/utils/data.py:63-78) along the SAMPLE axis.
    Tensors carry the sample on dim 0.  Collated lists come in two shapes: per-sample lists (`id`: B entries) and
    per-residue lists of per-sample tuples (`chain_id`, `icode`: L entries, each a tuple of B strings) -- the latter are
    sliced inside every tuple, never along the residue axis (which a plain `len(v) == B` test does whenever L == B)."""
    total = batch["aa"].shape[0]
    lo, hi = shard_bounds(total, world, rank)
    out = {}
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            out[k] = v[lo:hi] if v.dim() > 0 and v.shape[0] == total else v
        elif isinstance(v, (list, tuple)) and len(v) > 0 and all(isinstance(e, (list, tuple)) and len(e) == total for e in v):
            out[k] = [type(e)(e[lo:hi]) for e in v]
        elif isinstance(v, (list, tuple)) and len(v) == total:
            out[k] = v[lo:hi]
        else:
            out[k] = v
    return out, lo, hi


def shard_noise(noise, lo, hi):
    """the pre-drawn noise of the samples [lo, hi): expo [2N, B, L, 20] and gauss [N-1, B, L, 6] carry the sample on axis 1"""
    return {k: (v[:, lo:hi] if k in ("expo", "gauss") else v if k == "resample_u" else v[lo:hi]).contiguous() for k, v in noise.items() if v is not None}


def pack_state(step_dict):
    """dict of [B,L,...] tensors -> one fp32 [B,L,38] buffer (sequence ids are exact in fp32)."""
    B, L = step_dict["seqs"].shape
    parts = []
    for k, n in STATE_KEYS:
        parts.append(step_dict[k].reshape(B, L, n).to(torch.float32))
    return torch.cat(parts, dim=-1).contiguous()


def unpack_state(buf):
    B, L, _ = buf.shape
    out, o = {}, 0
    for k, n in STATE_KEYS:
        out[k] = buf[..., o:o + n]
        o += n
    out["rotmats"] = out["rotmats"].reshape(B, L, 3, 3)
    out["seqs"] = out["seqs"].reshape(B, L).round().to(torch.int64)
    return out


def all_gather_packed(local, sizes, group=None):
    """all-gather of per-rank [b_r, L, 38] buffers (ragged in b_r, b_r = 0 allowed) into [sum b_r, L, 38]."""
    world = dist.get_world_size(group)
    bmax = max(max(sizes), 1)
    pad = local
    if local.shape[0] < bmax:
        pad = torch.cat([local, local.new_zeros(bmax - local.shape[0], *local.shape[1:])], 0)
    pad = pad.contiguous()
    if pad.is_cuda and dist.get_backend(group) == "gloo":
        # gloo has no device all-gather (single-GPU dev boxes run the world-size-2 tests on it): staged through the host
        out = pad.new_empty(world * bmax, *pad.shape[1:], device="cpu")
        dist.all_gather_into_tensor(out, pad.cpu(), group=group)
        out = out.to(pad.device)
    else:
        out = pad.new_empty(world * bmax, *pad.shape[1:])
        dist.all_gather_into_tensor(out, pad, group=group)
    chunks = [out[r * bmax: r * bmax + sizes[r]] for r in range(world)]
    return torch.cat(chunks, 0)


def all_gather_final_state(sampler, group=None, sizes=None):
    """Gather the last trajectory slot of a DeviceSampler from every rank (device tensors, RCCL): ONE data collective.
    sizes: per-rank sample counts -- REQUIRED for ragged shards (contiguous shards of a known total: shard_bounds gives them
    without a collective, as sample_sharded does).  sizes=None means "every rank holds the same number of samples"
    (bench.py's weak-scaling replicas); that claim is CHECKED with one 2-int MIN/MAX all-reduce (set-up sized, 16 bytes) and a
    mismatch raises on every rank instead of handing RCCL buffers of different sizes (hang / corrupted rows)."""
    local = _final_state_of(sampler)
    world = dist.get_world_size(group)
    if sizes is None:
        n = int(local.shape[0])
        if world > 1:
            dev = local.device if dist.get_backend(group) != "gloo" else torch.device("cpu")
            mm = torch.tensor([n, -n], dtype=torch.int64, device=dev)
            dist.all_reduce(mm, op=dist.ReduceOp.MAX, group=group)
            nmax, nmin = int(mm[0].item()), -int(mm[1].item())
            if nmax != nmin:
                raise ValueError(f"all_gather_final_state(sizes=None) needs the same sample count on every rank, got {nmin}..{nmax}: "
                                 "pass sizes=[shard_bounds(total, world, r) widths] for ragged shards")
        sizes = [n] * world
    sizes = [int(s) for s in sizes]
    if len(sizes) != world or sizes[dist.get_rank(group)] != local.shape[0]:
        raise ValueError(f"sizes {sizes} do not describe this rank's {local.shape[0]} samples in a world of {world}")
    return unpack_state(all_gather_packed(local, sizes, group))


SEEDED_NOISE_VERSION = 2     # stream layout of seeded_noise: 1 = rounds 1-4 (four draws per sample), 2 = round 5 on (one normal block [L,27] +
                             # one uniform block [L,5] per sample).  Results of sample(seed=...) without explicit noise are comparable only
                             # between builds of the same version; tests/golden/f12_seeded_noise.npz pins version 2.


def seeded_noise(lo, hi, L, seed):
    """Initial noise of the GLOBAL samples [lo, hi) as a pure function of (seed, global sample index): one torch CPU
    generator per sample, so a shard draws exactly the rows the unsharded run draws, for every world size.
    The mapping (seed, sample) -> noise is VERSIONED (SEEDED_NOISE_VERSION) and pinned by a golden fixture: it is part of what a caller
    who passes seed= gets back, and it changed once (round 5).
    Two draws per sample (one normal block, one uniform block, split afterwards) and the quaternion -> rotation algebra once for the
    whole shard: the per-sample Python work is what a call pays on the host (round 4: four draws + ten small tensor ops per sample,
    5 - 15 ms per 64 samples)."""
    n = hi - lo
    nrm = torch.empty(max(n, 0), L, 27)                 # quaternion 4 | translation 3 | simplex 20
    uni = torch.empty(max(n, 0), L, 5)
    for k, i in enumerate(range(lo, hi)):
        g = torch.Generator().manual_seed((int(seed) * 1000003 + i) % (2 ** 63 - 1))
        nrm[k].normal_(generator=g)
        uni[k].uniform_(generator=g)
    # (the algebra and the slicing in numpy: single-threaded by construction -- see sampler.quat_to_rot_host)
    import numpy as np
    from .sampler import quat_to_rot_host
    a = nrm.numpy()
    return {"rot0": quat_to_rot_host(a[..., :4]), "trans0": torch.from_numpy(np.ascontiguousarray(a[..., 4:7])),
            "ang0": torch.from_numpy(uni.numpy() * np.float32(2 * math.pi)), "simplex0": torch.from_numpy(np.ascontiguousarray(a[..., 7:]))}


def _final_state_of(smp):
    eng = smp.eng
    B, L, last = eng.B, eng.L, smp.N - 1
    Lo = getattr(smp, "L_out", L)                      # (FlowModel.sample pads the residue axis to x16 internally)
    return pack_state({"rotmats": smp.traj_rot[last].view(B, L, 9)[:, :Lo], "trans": smp.traj_trans[last].view(B, L, 3)[:, :Lo],
                       "angles": smp.traj_ang[last].view(B, L, 5)[:, :Lo], "seqs_simplex": smp.traj_simplex[last].view(B, L, 20)[:, :Lo],
                       "seqs": smp.traj_seq[last].view(B, L)[:, :Lo]})


@torch.no_grad()
def sample_sharded(model, batch, num_steps=100, *, noise=None, seed=None, group=None, **kw):
    """FlowModel.sample over a batch sharded across the process group; returns the gathered FINAL state
    (dict of [B_total, L, ...] device tensors) on every rank.
    noise=None: the initial noise is drawn per GLOBAL sample index from `seed` (seeded_noise), so the result does not
    depend on the world size and equals `model.sample(batch, noise=None, seed=seed)` on one device.
    seed=None (default): a FRESH seed per call, like the reference's inference loop which draws new noise every time
    (flow_model.py:252-277) -- rank 0 draws it from torch's global CPU generator and broadcasts it (8 bytes, set-up, not on the
    data path), so repeated calls give different samples while all ranks agree; pass an explicit seed for full determinism.
    A rank whose shard is empty (B_total < world) skips sampling and contributes zero rows to the all-gather."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    if seed is None:
        st = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64)
        if world > 1:
            dev = batch["aa"].device if dist.get_backend(group) != "gloo" else torch.device("cpu")
            st = st.to(dev)
            dist.broadcast(st, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        seed = int(st.item())
    total, L = batch["aa"].shape[0], batch["aa"].shape[1]
    local, lo, hi = shard_batch(batch, world, rank)
    nz = shard_noise(noise, lo, hi) if noise is not None else seeded_noise(lo, hi, L, seed)
    sizes = [shard_bounds(total, world, r)[1] - shard_bounds(total, world, r)[0] for r in range(world)]
    if hi > lo:
        from .sampler import shard_cond_kwargs, shard_guide, shard_steer, shard_temper, steer_groups_of_shard
        kw = shard_cond_kwargs(kw, lo, hi, total)      # per-sample conditioning (row flags, allowed classes, start state): this shard's rows
        if kw.get("guide") is not None:
            kw["guide"] = shard_guide(kw["guide"], lo, hi, total)      # ... and this shard's hot spots and restraint lists
        if kw.get("temper") is not None:
            kw["temper"] = shard_temper(kw["temper"], lo, hi, total)    # ... and its temperature plane
        if kw.get("steer") is not None:                                # ... and its particle groups: whole ones only (ValueError otherwise)
            if nz.get("resample_u") is not None:                       # [N, G] by group: the columns of this shard's groups
                nz["resample_u"] = nz["resample_u"][:, steer_groups_of_shard(kw["steer"], lo, hi, total)].contiguous()
            kw["steer"] = shard_steer(kw["steer"], lo, hi, total)
        smp = model.sample(local, num_steps, noise=nz, seed=seed, first_sample=lo, return_sampler=True, **kw)
        if getattr(model, "last_steering", None) is not None:          # this rank's own records, sample indices made global
            model.last_steering["ancestors"] += lo
            model.last_steering["first_sample"] = lo
        packed = _final_state_of(smp)
    else:
        packed = torch.zeros(0, L, PACK_WIDTH, dtype=torch.float32, device=batch["aa"].device)
    return unpack_state(all_gather_packed(packed, sizes, group))


def allreduce_flat(flat, dist=None):
    """Average one flat gradient buffer over the replicas IN PLACE (the gradient arena of the graph-captured training step:
    every `.grad` is a view of it, so there is no flatten and no copy-back).  No-op for a single replica."""
    if dist is None:
        import torch.distributed as dist
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
        flat /= dist.get_world_size()
    return flat.numel()


def allreduce_gradients(parameters, dist=None):
    """Data-parallel training step (train_ddp.py:94 wraps the model in DDP): average the gradients of the
    replicas with ONE all-reduce over a flat fp32 bucket (6.88 M parameters = 27.5 MB; on the xGMI mesh one large
    collective beats per-tensor ones).  Works on any backend (RCCL on the GPU box, gloo in the CPU tests).
    Returns the number of elements reduced."""
    import torch
    if dist is None:
        import torch.distributed as dist
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return 0
    if not (dist.is_initialized() and dist.get_world_size() > 1):
        return sum(p.grad.numel() for p in params)              # one replica: the average is the gradient itself
    flat = torch.cat([p.grad.reshape(-1).to(torch.float32) for p in params])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    flat /= dist.get_world_size()
    o = 0
    for p in params:
        n = p.grad.numel()
        p.grad.copy_(flat[o:o + n].view_as(p.grad))
        o += n
    return o
