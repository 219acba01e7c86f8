"""GPU: gradient accumulation and global-norm clipping on the data-parallel path (workers as in tests/test_hip_ddp.py: two
gloo ranks sharing cuda:0, and one nccl rank whose all-reduces are RCCL kernels).  There is no ``no_sync``: every backward
of a window runs its all-reduce round, averaging already-averaged sums is exact, and after the last round the gradients
are identical on every rank, so the clip needs no collective."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _plain(dev, **kw):
    sys.path.insert(0, ROOT)
    from paradis_model_amd.config import reduced_config, stub_datamodule
    from paradis_model_amd.harness import TrainStep, make_grids
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.model import Paradis
    cfg = reduced_config()
    lat_deg, lg, og = make_grids(16, 32, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).to(dev)
    return model, TrainStep(model, build_loss(cfg, lat_deg).to(dev), cfg, **kw)


def _flat(model):
    return torch.cat([p.detach().flatten() for p in model.parameters()]).cpu()


# ================================================================================================ two ranks, a window
def _window_worker(rank, world, port, out_dir, clip_val):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from paradis_model_amd.config import reduced_config, stub_datamodule
    from paradis_model_amd.harness import TrainStep, init_distributed, make_grids, synthetic_batch, wrap_ddp
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.model import Paradis
    init_distributed("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = reduced_config()
    lat_deg, lg, og = make_grids(16, 32, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).to(dev)
    ddp = wrap_ddp(model, bucket_cap_mb=0.1, device_ids=[0])
    step = TrainStep(ddp, build_loss(cfg, lat_deg).to(dev), cfg, accumulate_grad_batches=2, gradient_clip_val=clip_val)
    shards = []
    for i in range(2):
        full = synthetic_batch(16, 32, False, 2 * world, 1, seed=5 + i, device=dev)
        shards.append(tuple(t[rank * 2:(rank + 1) * 2] for t in full))
    losses, norms = [], []
    for _ in range(2):
        losses.append(step.window(shards).tolist())
        norms.append(step.last_grad_norm.cpu().clone())
    torch.save({"params": _flat(model), "losses": losses, "norms": norms, "opt_steps": step.opt_steps},
               os.path.join(out_dir, f"rank{rank}.pt"))
    torch.distributed.destroy_process_group()


def test_two_rank_window_with_clipping_matches_single_process(tmp_path):
    sys.path.insert(0, ROOT)
    from paradis_model_amd.harness import synthetic_batch
    world = 2
    dev = torch.device("cuda", 0)
    micro = [synthetic_batch(16, 32, False, 2 * world, 1, seed=5 + i, device=dev) for i in range(2)]
    # the clip value: half the first window's norm of an unclipped single-process twin
    _, probe = _plain(dev, accumulate_grad_batches=2, gradient_clip_val=1e30)
    probe.window(micro)
    clip_val = 0.5 * float(probe.last_grad_norm[0])
    assert clip_val > 0
    mp.spawn(_window_worker, args=(world, _free_port(), str(tmp_path), clip_val), nprocs=world, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert torch.equal(r0["params"], r1["params"])
    assert all(torch.equal(a, b) for a, b in zip(r0["norms"], r1["norms"]))
    assert r0["opt_steps"] == 2
    assert float(r0["norms"][0][1]) < 1.0                          # the clip bites on the first window
    # one process on the concatenated micro-batches
    model, step = _plain(dev, accumulate_grad_batches=2, gradient_clip_val=clip_val)
    losses = [step.window(micro).tolist() for _ in range(2)]
    for w in range(2):
        for k in range(2):
            a = losses[w][k]
            assert abs(a - 0.5 * (r0["losses"][w][k] + r1["losses"][w][k])) < 1e-5 * abs(a)
    flat = _flat(model)
    assert float((flat - r0["params"]).abs().max()) < 5e-4
    assert float((flat - r0["params"]).abs().mean()) < 2e-5


# ================================================================================================ one rank, RCCL
N_STEPS = 14


def _nccl_worker(rank, port, out_dir, graphed, clip_val):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from paradis_model_amd.config import reduced_config, stub_datamodule
    from paradis_model_amd.harness import GraphedTrainStep, TrainStep, make_grids, synthetic_batch, wrap_ddp
    from paradis_model_amd.loss import build_loss
    from paradis_model_amd.model import Paradis
    os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    dev = torch.device("cuda", 0)
    cfg = reduced_config()
    lat_deg, lg, og = make_grids(16, 32, False)
    torch.manual_seed(42)
    model = Paradis(stub_datamodule(cfg), cfg, lg, og).to(dev)
    ddp = wrap_ddp(model, bucket_cap_mb=0.1, device_ids=[0], force=True, capturable=graphed)
    assert isinstance(ddp, torch.nn.parallel.DistributedDataParallel)
    loss_fn = build_loss(cfg, lat_deg).to(dev)
    batches = [synthetic_batch(16, 32, False, 2, 1, seed=5 + i, device=dev) for i in range(2)]
    rec = {}
    if graphed:
        # a window under capture is not supported with DDP yet: refused before anything runs
        windowed = TrainStep(ddp, loss_fn, cfg, capturable=True, accumulate_grad_batches=2, gradient_clip_val=clip_val)
        try:
            GraphedTrainStep(windowed, batches)
            rec["refusal"] = None
        except ValueError as e:
            rec["refusal"] = str(e)
        del windowed
    step = TrainStep(ddp, loss_fn, cfg, capturable=graphed, gradient_clip_val=clip_val)
    W = GraphedTrainStep.DDP_WARMUP
    order = [0] * W + [i % 2 for i in range(N_STEPS - W)]
    if graphed:
        g = GraphedTrainStep(step, batches[0], warmup=2)
        losses = [float(g(batches[i])) for i in order[W:]]
    else:
        losses = [float(step(batches[i])) for i in order]
    torch.cuda.synchronize()
    rec.update(params=_flat(model), losses=losses, norm=step.last_grad_norm.cpu().clone())
    torch.save(rec, os.path.join(out_dir, f"nccl_{int(graphed)}.pt"))
    # ordered teardown: a captured graph holds RCCL nodes - it goes before the communicator does
    if graphed:
        del g
    del step, ddp
    import gc
    gc.collect()
    torch.cuda.synchronize()
    dist.destroy_process_group()


def test_one_rank_nccl_with_clipping_eager_and_graphed_match_plain(tmp_path):
    sys.path.insert(0, ROOT)
    from paradis_model_amd.harness import GraphedTrainStep, synthetic_batch
    from tests._util import max_rel
    dev = torch.device("cuda", 0)
    batches = [synthetic_batch(16, 32, False, 2, 1, seed=5 + i, device=dev) for i in range(2)]
    _, probe = _plain(dev, gradient_clip_val=1e30)
    probe(batches[0])
    clip_val = 0.5 * float(probe.last_grad_norm[0])
    assert clip_val > 0
    mp.spawn(_nccl_worker, args=(_free_port(), str(tmp_path), False, clip_val), nprocs=1, join=True)
    mp.spawn(_nccl_worker, args=(_free_port(), str(tmp_path), True, clip_val), nprocs=1, join=True)
    e, g = torch.load(tmp_path / "nccl_0.pt"), torch.load(tmp_path / "nccl_1.pt")
    # graphed DDP with a window of two: the ValueError names the combination
    assert g["refusal"] is not None and "DistributedDataParallel" in g["refusal"] \
        and "accumulate_grad_batches" in g["refusal"], g["refusal"]
    # plain twin in this process
    model, step = _plain(dev, gradient_clip_val=clip_val)
    W = GraphedTrainStep.DDP_WARMUP
    order = [0] * W + [i % 2 for i in range(N_STEPS - W)]
    losses = []
    for k, i in enumerate(order):
        losses.append(float(step(batches[i])))
        if k == 0:
            assert float(step.last_grad_norm[1]) < 1.0             # the clip bites on the first step
    flat = _flat(model)
    norm = step.last_grad_norm.cpu()
    assert max_rel(e["params"], flat) <= 1e-6, max_rel(e["params"], flat)
    assert max_rel(g["params"], flat) <= 1e-6, max_rel(g["params"], flat)
    for a, b in zip(losses, e["losses"]):
        assert abs(a - b) <= 1e-6 * abs(a), (losses, e["losses"])
    for a, b in zip(losses[W:], g["losses"]):
        assert abs(a - b) <= 1e-6 * abs(a), (losses, g["losses"])
    for other in (e["norm"], g["norm"]):
        assert max_rel(other, norm) <= 1e-6, (other, norm)
