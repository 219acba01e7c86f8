"""Host-side callers of the hot path (e): synthetic ERA5-shaped
batches, the autoregressive training step of the reference's ``LitParadis.training_step``
(reference ``trainer.py:498-587`` + ``_autoregression_next_input`` ``:710-729``) restated without
Lightning, and the data-parallel wrapper (one process per GPU, RCCL all-reduce overlapped with
backward through ``torch.nn.parallel.DistributedDataParallel``).

Everything here is device agnostic plumbing (tensor concatenation, optimiser, collectives); the
compute is inside the model that is passed in.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence, Tuple

import torch
import torch.distributed as dist

# ---------------------------------------------------------------------------------- grids / data
GRID_PRESETS = {
    "5.625deg": (32, 64, False),    # WeatherBench2 64x32 equiangular, no pole rows
    "1.40625deg": (128, 256, False),
    "0.25deg": (721, 1440, True),   # with pole rows
}


def make_grids(nlat: int, nlon: int, poles: bool):
    """(lat_deg[H], lat_grid[H,W], lon_grid[H,W]) in fp32 radians, latitude ascending
    (reference data/era5_dataset.py:77-81,178-182)."""
    if poles:
        lat = torch.linspace(-90.0, 90.0, nlat, dtype=torch.float64)
    else:
        d = 180.0 / nlat
        lat = -90.0 + d / 2 + d * torch.arange(nlat, dtype=torch.float64)
    lon = torch.arange(nlon, dtype=torch.float64) * (360.0 / nlon)
    lat32, lon32 = lat.to(torch.float32), lon.to(torch.float32)
    lg, og = torch.meshgrid(torch.deg2rad(lat32), torch.deg2rad(lon32), indexing="ij")
    return lat32, lg.contiguous(), og.contiguous()


def synthetic_batch(nlat: int, nlon: int, poles: bool, batch: int, steps: int, *, seed: int = 1234,
                    device="cpu", n_dyn: int = 166, n_out: int = 97, n_forc: int = 10):
    """ERA5-shaped batch tuple exactly as the reference dataset yields it after collation
    (reference data/era5_dataset.py:379-382): input [B,1,166,H,W] ~ N(0,1), target [B,S,97,H,W] ~
    N(0,1), forcings [B,S,H,W,10] ~ U(-1,1), constants [B,1,H,W,10] = 4 random fields, z-scored
    inverse lon spacing, cos(lat), cos(lon), sin(lon), lat, lon."""
    g = torch.Generator().manual_seed(seed)
    _, lg, og = make_grids(nlat, nlon, poles)
    inp = torch.randn(batch, 1, n_dyn, nlat, nlon, generator=g)
    tgt = torch.randn(batch, steps, n_out, nlat, nlon, generator=g)
    forc = torch.rand(batch, steps, nlat, nlon, n_forc, generator=g) * 2 - 1
    rnd = torch.randn(4, nlat, nlon, generator=g)
    dlon = math.radians(360.0 / nlon)
    inv = 1.0 / (2 * torch.arcsin(torch.cos(lg) ** 2 * math.sin(dlon / 2)).clamp_min(1e-12) * 6371)
    inv = (inv - inv.mean()) / inv.std()
    const = torch.stack([*rnd, inv, torch.cos(lg), torch.cos(og), torch.sin(og), lg, og])
    const = const.permute(1, 2, 0).unsqueeze(0).unsqueeze(0).expand(batch, 1, -1, -1, -1).contiguous()
    return tuple(t.to(device) for t in (inp, tgt, forc, const))


# ---------------------------------------------------------------------------------- rollout
def assemble_model_input(input_data, forcings_step, constants):
    """cat([input[B,1,166,H,W], forcings[B,1,10,H,W], constants[B,1,10,H,W]], 2).squeeze(1)
    (reference trainer.py:534-538)."""
    if input_data.is_cuda:
        from . import ops   # strided block copies by the HIP library (no ATen cat / permute copies)
        return ops.concat_channels([input_data.squeeze(1), forcings_step.squeeze(1), constants.squeeze(1)])
    return torch.cat([input_data, forcings_step, constants], dim=2).squeeze(1)


def next_input(model_input, output, num_common: int, n_inputs: int):
    """Autoregressive channel stack update (reference trainer.py:710-729)."""
    common = output[:, :num_common]
    if n_inputs == 1:
        return common
    if model_input.is_cuda:
        from . import ops
        return ops.concat_channels([model_input[:, num_common:num_common * n_inputs], common])
    return torch.cat([model_input[:, num_common:num_common * n_inputs], common], dim=1)


def rollout_loss(model, loss_fn, batch, *, num_common: int, n_inputs: int, accum: int = 1,
                 detach_every: Optional[int] = None, keep_outputs: bool = False,
                 backward: bool = True, amp: bool = False, on_step=None):
    """The autoregressive hot loop of ``training_step`` (reference trainer.py:508-576): per step
    assemble the input, run the model, accumulate ``loss/(S*accum)``, feed the prediction back;
    ``backward`` at chunk ends (every ``detach_every`` steps and at the last step), detaching the
    carried input.  Returns (sum of chunk losses as a detached tensor, outputs if requested).

    ``amp``: the forward and the loss of every step run under ``torch.autocast(bfloat16)``; the ``backward`` calls run
    OUTSIDE the autocast region, as under Lightning's ``precision="bf16-mixed"`` plugin (reference train.py:56) and
    as the PyTorch AMP recipe prescribes.

    ``on_step``: called with ``(out, true_data[:, step])`` after each step's loss (the per-channel training losses of
    ``diagnostics.TrainStats``, reference trainer.py:544-556); it takes no part in the loss."""
    input_data, true_data, forcings, constant_data = batch
    constants = constant_data[:, :1].permute(0, 1, 4, 2, 3)
    forcings = forcings.permute(0, 1, 4, 2, 3)
    S = true_data.size(1)
    total = torch.zeros((), device=input_data.device)
    chunk = 0.0
    outs = []
    for step in range(S):
        with torch.autocast("cuda" if input_data.is_cuda else "cpu", dtype=torch.bfloat16, enabled=bool(amp)):
            mi = assemble_model_input(input_data, forcings[:, step].unsqueeze(1), constants)
            out = model(mi)
            if keep_outputs:
                outs.append(out.detach())
            chunk = chunk + loss_fn(out, true_data[:, step]) / (S * accum)
            if on_step is not None:
                on_step(out, true_data[:, step])
            input_data = next_input(mi, out, num_common, n_inputs).unsqueeze(1)
        if (detach_every is not None and (step + 1) % detach_every == 0) or step == S - 1:
            if backward:
                chunk.backward()
            total = total + chunk.detach()
            input_data = input_data.detach()
            chunk = 0.0
    return total, outs


def _wgrad_side_stream() -> bool:
    """is the opt-in side stream of the weight-gradient GEMMs on (``ops.WgradSide``, PARADIS_WGRAD_STREAM=1)"""
    import sys
    ops = sys.modules.get(__package__ + ".ops")
    if ops is not None:
        return bool(ops.WgradSide.enabled)
    return os.environ.get("PARADIS_WGRAD_STREAM", "0") == "1"


class TrainStep:
    """forward(S rollout steps) + ParadisLoss + backward + AdamW, the unit the benchmark times
    (SURVEY.md section 8d).  AdamW hyper-parameters follow reference trainer.py:327-335.

    ``stats``: a ``diagnostics.TrainStats`` - the reference's ``log_additional_stats`` (trainer.py:520-556, 844-923): the
    per-channel losses of every rollout step, the gradient statistics between the backward (DDP's all-reduces are
    finished) and the optimiser step, and the step loss; read with ``stats.result()``.  ``None``: nothing is added.

    ``schedule``: a ``(lr_lambda, total_steps)`` pair or what ``schedule.from_config`` returns - the reference's
    ``LambdaLR`` with interval ``"step"`` (trainer.py:416-456), tabulated once (``schedule.DeviceSchedule``).  A capturable
    optimiser reads the table on the device, one launch inside ``opt.step()`` (so inside a captured graph); any other
    optimiser gets ``group["lr"]`` set from the same table before every ``opt.step()``.  ``None``: the learning rate is
    whatever ``group["lr"]`` holds.  Schedules advance per optimiser step, not per call.

    ``accumulate_grad_batches`` (``None``: ``cfg.training.accumulate_grad_batches``, default 1): a call is ONE micro-batch
    with the reference's gating (trainer.py:503-506, 560, 578-587) on the number of micro-batches since the last optimiser
    step: the gradients are zeroed on the first batch of a window, the loss is divided by ``S * N``, and the optimiser (and
    the schedule) step on the N-th.  A call returns the reference's ``train_loss`` of its batch (trainer.py:589: the rollout
    mean WITHOUT the 1/N).  ``pending``: micro-batches accumulated since the last optimiser step; ``flush()``: the
    reference's ``is_last_batch`` - steps with what is there (the gradients still carry 1/N); ``window(batches)``: N calls,
    the stacked ``[N]`` losses.

    ``gradient_clip_val`` (``None``: ``cfg.training.gradient_clip_val``; ``None`` or 0: off, Lightning's rule): global-norm
    clipping (``clip.clip_grad_norm_``, reference train.py:52-53) of every parameter of ``opt.param_groups`` that has a
    gradient, between the last backward (and the statistics, which see the unclipped gradients: Lightning's hook order)
    and the optimiser step.  ``last_grad_norm``: fp32 ``[2]`` on the device, ``{norm before clipping, coefficient}`` of the
    most recent optimiser step; ``None`` with clipping off.

    With N = 1 and clipping off the step launches exactly what it launched before these two controls existed."""

    def __init__(self, model, loss_fn, cfg, *, num_common: int = 83, n_inputs: int = 2, fused=None,
                 capturable: bool = False, amp: bool = False, stats=None, schedule=None,
                 accumulate_grad_batches=None, gradient_clip_val=None):
        self.model, self.loss_fn = model, loss_fn
        self.stats = stats
        if accumulate_grad_batches is None:
            accumulate_grad_batches = cfg.training.get("accumulate_grad_batches", 1)
        if gradient_clip_val is None:
            gradient_clip_val = cfg.training.get("gradient_clip_val", None)
        if isinstance(accumulate_grad_batches, bool) or not isinstance(accumulate_grad_batches, int) \
                or accumulate_grad_batches < 1:
            raise ValueError(f"accumulate_grad_batches must be an int >= 1, got {accumulate_grad_batches!r}")
        self.accumulate = accumulate_grad_batches
        if gradient_clip_val is not None:
            gradient_clip_val = float(gradient_clip_val)
            if not math.isfinite(gradient_clip_val) or gradient_clip_val < 0:
                raise ValueError(f"gradient_clip_val must be finite and >= 0, got {gradient_clip_val!r}")
        self.clip_val = gradient_clip_val or None          # None or 0: off
        if self.accumulate > 1 and stats is not None:
            raise ValueError("stats= together with accumulate_grad_batches > 1: per-window statistics are not supported")
        if self.accumulate > 1 and _wgrad_side_stream():
            raise ValueError("accumulate_grad_batches > 1 with PARADIS_WGRAD_STREAM=1: the side stream hands its "
                             "gradients over safely only while .grad is None")
        self.pending = 0              # micro-batches accumulated since the last optimiser step
        self.last_grad_norm = None
        self._clip_plan = None
        # amp: forward and loss under torch.autocast(bfloat16) - the reference's shipped ``use_amp: true`` /
        # ``precision="bf16-mixed"`` (config/paradis_settings.yaml:75, train.py:56); parameters, gradients and the
        # optimiser stay fp32, as with Lightning's mixed-precision plugin
        self.amp = bool(amp)
        self.num_common, self.n_inputs = num_common, n_inputs
        o = cfg.training.optimizer
        params = [p for p in model.parameters() if p.requires_grad]
        on_hip = bool(params and params[0].is_cuda)
        name = o.get("name", "adamw")
        if "muon" in name:
            # reference trainer.py:337-364 (dion.Muon / dion.NorMuon over build_param_groups)
            if not on_hip:
                raise RuntimeError("Muon/NorMuon run on the HIP device only")
            from . import optim
            inner = model.module if hasattr(model, "module") else model
            groups = optim.build_param_groups(inner, lr=o.lr, weight_decay=o.weight_decay, optimizer_name=name)
            cls = {"muon": optim.Muon, "normuon": optim.NorMuon}.get(name)
            if cls is None:
                raise ValueError(f"Optimizer {name} not supported. Choose between normuon|muon")
            self.opt = cls(groups, lr=o.lr, weight_decay=o.weight_decay, betas=(o.beta1, o.beta2),
                           use_triton=True, capturable=capturable)
        elif on_hip and fused is None:
            from .optim import AdamW   # HIP kernel, torch.optim.AdamW semantics
            self.opt = AdamW(params, lr=o.lr, weight_decay=o.weight_decay, betas=(o.beta1, o.beta2),
                             capturable=capturable)
        else:
            self.opt = torch.optim.AdamW(params, lr=o.lr, weight_decay=o.weight_decay,
                                         betas=(o.beta1, o.beta2), fused=bool(fused))
        self.detach_every = o.get("detach_gradient_every", None)
        self.schedule = None          # the host-driven table (non-capturable optimiser); a capturable one owns its own
        self.opt_steps = 0            # optimiser steps taken through this object
        if schedule is not None:
            from .schedule import DeviceSchedule, as_schedule
            sch = as_schedule(schedule)
            table = DeviceSchedule(self.opt, sch.lr_lambda, sch.total_steps)
            if getattr(self.opt, "capturable", False):
                self.opt.attach_schedule(table)
            else:
                self.schedule = table

    def __call__(self, batch):
        N = self.accumulate
        if self.pending == 0:
            self.opt.zero_grad(set_to_none=True)
        stats = self.stats
        if stats is None:
            loss, _ = rollout_loss(self.model, self.loss_fn, batch, num_common=self.num_common, accum=N,
                                   n_inputs=self.n_inputs, detach_every=self.detach_every, amp=self.amp)
        else:
            stats.begin_step()
            loss, _ = rollout_loss(self.model, self.loss_fn, batch, num_common=self.num_common,
                                   n_inputs=self.n_inputs, detach_every=self.detach_every, amp=self.amp,
                                   on_step=stats.on_rollout_step)
        self.pending += 1
        if self.pending == N:
            if stats is not None:
                stats.before_optimizer_step(self.opt)      # in front of the clip: the statistics see unclipped gradients
                stats.record_loss(loss)
            self._optimizer_step()
        return loss if N == 1 else loss * N

    def _optimizer_step(self):
        if self.clip_val is not None:
            self.last_grad_norm = self._clip()
        if self.schedule is not None:
            for gi, group in enumerate(self.opt.param_groups):
                group["lr"] = self.schedule.host_lr(gi, self.opt_steps)
        self.opt.step()
        self.opt_steps += 1
        self.pending = 0

    def _clip(self):
        from . import clip
        params = [p for group in self.opt.param_groups for p in group["params"]]
        if params and params[0].is_cuda:
            # the step owns its plan instead of taking ``clip.plan_for``'s: a captured graph reads this plan's tables and
            # ``out`` on every replay, so the small global cache must never be able to evict (free) it
            key = tuple((id(p), p.numel()) for p in params) + (str(params[0].device),)
            if self._clip_plan is None or self._clip_plan[0] != key:
                self._clip_plan = (key, clip.ClipPlan([p.numel() for p in params], params[0].device))
            return clip.clip_grad_norm_(params, self.clip_val, plan=self._clip_plan[1])
        return clip.clip_grad_norm_(params, self.clip_val)

    @property
    def clip_plan(self):
        """the ``clip.ClipPlan`` of this step's clipping on the HIP device (``None`` before the first clipped step)"""
        return None if self._clip_plan is None else self._clip_plan[1]

    def flush(self) -> bool:
        """the reference's ``is_last_batch`` (trainer.py:578-587): an optimiser step on the micro-batches accumulated so
        far, if any (their gradients still carry the 1/N of a full window); returns whether it stepped"""
        if self.pending == 0:
            return False
        self._optimizer_step()
        return True

    def window(self, batches):
        """one whole accumulation window: ``len(batches) == accumulate_grad_batches`` calls, the stacked ``[N]`` losses"""
        batches = list(batches)
        if self.pending != 0:
            raise ValueError(f"window(): {self.pending} micro-batches are pending; flush() first")
        if len(batches) != self.accumulate:
            raise ValueError(f"window(): {len(batches)} batches for accumulate_grad_batches = {self.accumulate}")
        return torch.stack([self(b) for b in batches])


class GraphedTrainStep:
    """The whole training step - forward (S rollout steps), ParadisLoss, backward, optimiser (AdamW, Muon or NorMuon, with
    or without a device-side learning-rate schedule): ~2,500 kernel launches -
    captured once into a HIP graph (``torch.cuda.CUDAGraph``) and replayed: the host enqueues one graph launch per
    step instead of walking dispatcher -> autograd -> Python kernel -> ctypes for every op (23.5 ms of host time per
    step at 32x64, the bound below ~4 samples per GPU).  Everything on the path is capture-safe: the ops launch on
    the current stream through the C ABI without host synchronisation, workspaces come from the caching allocator
    (the graph's private pool under capture), and the optimiser's step count and learning rate live on the device
    (``optim.AdamW(capturable=True)``, and the same flag of ``optim.Muon`` / ``optim.NorMuon``).  A schedule given to the
    ``TrainStep`` is a launch inside the optimiser step that reads the DEVICE step count, so the replayed learning rates
    are those of an eager run: the capture advances only host counters, and the first replay does not advance them again.

    ``step`` must be a ``TrainStep(..., capturable=True)``; ``example_batch`` fixes the shapes.  ``warmup`` eager
    steps run first on a side stream (they are real optimiser steps: kernel attributes, optimiser state and the
    allocator's pools must exist before capture).

    Data parallel: a model wrapped by ``wrap_ddp(..., capturable=True)`` is captured WITH its gradient all-reduces -
    RCCL collectives are capturable, the Reducer launches them from its autograd hooks onto the process group's
    stream, which forks from and joins the capturing stream inside the capture.  What that needs (PyTorch's CUDA-graph
    notes for DDP): the wrapper constructed on a side stream, at least 11 eager DDP iterations before the capture (the
    Reducer rebuilds its buckets after the first one and settles its bookkeeping over the next ones), and no
    asynchronous NCCL error handling thread touching the captured work (TORCH_NCCL_ASYNC_ERROR_HANDLING=0, set by
    ``init_distributed(capturable=True)``).

    Gradient clipping (``TrainStep(gradient_clip_val=...)``) and truncated BPTT (``detach_gradient_every``) are simply
    captured with the step.  With ``accumulate_grad_batches`` = N > 1 the unit of capture is the WINDOW: ``example_batch``
    is a sequence of N batches, ``__call__(batches)`` copies N batches into the static buffers, makes ONE replay and returns
    the static ``[N]`` losses; ``eager_step(batches)`` runs ``TrainStep.window``.  A DDP-wrapped model with N > 1 is not
    supported under capture yet (eager DDP with N > 1 works as in the reference: one all-reduce round per backward).

    Feeding the static buffers in place: ``__call__`` skips the copy of a tensor that already IS its static buffer, so a
    ``dataset.DeviceDataset`` can assemble every batch straight into them -

        for idx in index_batches:                       # device int64 vectors, e.g. slices of one epoch permutation
            ds.batch(idx, out=g.static_batch)           # one assembly launch + the forcings launch, no host sync
            loss = g(g.static_batch)                    # no copies: one graph replay

    (``tests/test_hip_dataset.py::test_graphed_train_step_fed_in_place``)."""

    DDP_WARMUP = 11

    def __init__(self, step: TrainStep, example_batch, warmup: int = 2):
        if not getattr(step.opt, "capturable", False):
            raise ValueError("GraphedTrainStep needs TrainStep(..., capturable=True)")
        self.windowed = step.accumulate > 1
        if isinstance(step.model, torch.nn.parallel.DistributedDataParallel):
            if self.windowed:
                raise ValueError("GraphedTrainStep: a DistributedDataParallel model with accumulate_grad_batches > 1 is "
                                 "not supported under capture yet")
            warmup = max(warmup, self.DDP_WARMUP)
        if step.pending != 0:
            raise ValueError(f"GraphedTrainStep: {step.pending} micro-batches are pending; flush() first")
        self.step = step
        if self.windowed:
            example_batch = list(example_batch)
            if len(example_batch) != step.accumulate or not all(isinstance(b, (tuple, list)) for b in example_batch):
                raise ValueError(f"GraphedTrainStep: example_batch must be a sequence of {step.accumulate} batches "
                                 "(accumulate_grad_batches)")
            self.static_batch = [tuple(t.clone() for t in b) for b in example_batch]
            run = step.window
        else:
            self.static_batch = tuple(t.clone() for t in example_batch)
            run = step
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):
                run(self.static_batch)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.warmup_steps = max(1, warmup)
        self.graph = torch.cuda.CUDAGraph()
        step.opt.zero_grad(set_to_none=True)
        # With a process group alive, RCCL's watchdog thread polls its work events (hipEventQuery) whenever it likes; under the
        # default capture mode ("global") such a call from ANY thread while this one captures is an error that kills the
        # process ("operation not permitted when stream is capturing": seen once in ~10 runs of the 1-rank nccl test).
        # "thread_local" checks the capturing thread only.
        import torch.distributed as dist
        with_pg = dist.is_available() and dist.is_initialized()
        mode = "thread_local" if with_pg else "global"
        if with_pg:
            # ... and give the watchdog two of its 100 ms rounds to retire the work items of the eager warm-up iterations
            # (all complete: the device is synchronised), so that it holds no event to poll while the capture runs
            import time as _time
            _time.sleep(0.25)
        with torch.cuda.graph(self.graph, capture_error_mode=mode):
            self.static_loss = run(self.static_batch)
        # the graph's optimiser nodes copy the pinned pointer tables of the capture on every replay: keep a snapshot
        # (and the captured gradient tensors, which live in the graph's private pool) for eager_step()
        self._tables = step.opt.snapshot_pointer_tables()
        stats = getattr(step, "stats", None)      # the statistics launches were captured with the step: same for their table
        self._stats_table = stats.snapshot_pointer_tables() if stats is not None else None
        plan = step.clip_plan                     # ... and for the gradient address row of the clip
        self._clip_table = plan.snapshot_pointer_tables() if plan is not None else None
        self._captured_grads = [p.grad for g in step.opt.param_groups for p in g["params"]]
        # the capture ran the Python side of one step (host step counts advanced) without executing it on the
        # device: bring the device-side count of the captured tick back in line on first replay
        self._first = True
        self._replayed = torch.cuda.Event()

    def _pairs(self, batch):
        """(static batch, given batch) pairs: one, or the N of a window"""
        if not self.windowed:
            return [(self.static_batch, batch)]
        batch = list(batch)
        if len(batch) != len(self.static_batch):
            raise ValueError(f"GraphedTrainStep: {len(batch)} batches for a window of {len(self.static_batch)}")
        return list(zip(self.static_batch, batch))

    def __call__(self, batch):
        for static, given in self._pairs(batch):
            for dst, src in zip(static, given):
                if dst.data_ptr() != src.data_ptr():
                    dst.copy_(src, non_blocking=True)
        if self._first:
            self._first = False      # host counters already include this step (incremented during capture)
        else:
            self.step.opt.note_replayed()
            self.step.opt_steps += 1
        self.graph.replay()
        self._replayed.record()      # eager_step() waits for it before it touches the optimiser's pointer tables
        # the replay rewrites the parameters through raw pointers: no autograd version bump, no optimiser post-hook.
        # Without this an eager forward between replays (validation) would keep using the split weight images it
        # cached at the previous epoch.
        from . import ops
        ops.weights_updated()
        return self.static_loss

    def eager_step(self, batch):
        """A real (un-captured) optimiser step on ``batch`` - e.g. an odd-shaped last batch of an epoch.  The
        captured graph reads the gradient / moment addresses of ITS step from the optimiser's pinned pointer table;
        an eager step rewrites that table (its gradients are fresh allocations), so the table is restored afterwards
        and the gradients of the capture stay alive (``TrainStep`` keeps them: see ``_captured_grads``).

        ``graph.replay()`` is asynchronous and the captured optimiser node re-reads the pinned table WHEN THE GPU REACHES
        IT: an eager step issued right behind a replay would overwrite the table under a replay that has not got
        there yet (any GPU-bound configuration: ~150 ms of device time against ~30 ms of host enqueue), and that
        replay would apply AdamW with the eager step's gradient addresses.  So the host first waits for the last
        replay to finish (``tests/test_hip_graph.py::test_eager_step_right_behind_a_gpu_bound_replay``).
        The pinned address table of a ``TrainStep(stats=...)``'s statistics and the address row of its clip are
        snapshotted and restored the same way.  With ``accumulate_grad_batches`` > 1, ``batch`` is a window of N batches
        (``TrainStep.window``) and the ``[N]`` losses are returned."""
        self._replayed.synchronize()
        loss = self.step.window(batch) if self.windowed else self.step(batch)
        self.step.opt.restore_pointer_tables(self._tables)
        if self._stats_table is not None:
            self.step.stats.restore_pointer_tables(self._stats_table)
        if self._clip_table is not None:
            self.step.clip_plan.restore_pointer_tables(self._clip_table)
        return loss


# ---------------------------------------------------------------------------------- graphed forward
def capture_forward(fn, warmup: int = 2):
    """Capture the no-grad callable ``fn()`` into a HIP graph: ``warmup`` eager calls on a side stream (kernel attributes,
    lazily built geometry and the allocator's pools must exist before capture), then one captured call.  Returns
    (graph, what the captured call returned - static tensors in the graph's pool, overwritten by every replay).
    Capture mode as ``GraphedTrainStep``: "global" unless a process group is alive."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(1, warmup)):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with_pg = dist.is_available() and dist.is_initialized()
    if with_pg:
        import time as _time
        _time.sleep(0.25)            # see GraphedTrainStep: let RCCL's watchdog retire its work items first
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local" if with_pg else "global"):
        out = fn()
    return graph, out


class GraphedForward:
    """The no-grad forward of ``model`` on inputs shaped like ``example_input`` as one HIP-graph replay (one host call
    instead of one per kernel: what a host-bound small-batch forward needs).  ``__call__(x) -> y``; ``y`` is
    a static tensor that the next call overwrites.  Captured outside ``ops.frozen_weights()``: the weight-image kernels
    are nodes of the graph, so parameters written in place (``load_state_dict``, an optimiser step) are honoured by the
    next replay without re-capture.  Works under ``torch.no_grad()`` and ``torch.inference_mode()``: the static tensors
    are created outside inference mode."""

    def __init__(self, model, example_input, warmup: int = 2):
        from . import ops
        self.model = model
        with torch.inference_mode(False), torch.no_grad(), ops.frozen_weights(False):
            self.static_input = torch.empty_like(example_input).copy_(example_input)
            self.graph, self.static_output = capture_forward(lambda: model(self.static_input), warmup)

    def __call__(self, x):
        if x.data_ptr() != self.static_input.data_ptr():
            self.static_input.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.static_output


# ---------------------------------------------------------------------------------- data parallel
def init_distributed(backend: Optional[str] = None, capturable: bool = False) -> Tuple[int, int, int]:
    """(rank, local_rank, world) from the torchrun environment; no-op for a single process.

    ``capturable``: the DDP step will be captured into a HIP graph (``GraphedTrainStep``): a replay runs its RCCL
    kernels without the watchdog's bookkeeping, so the asynchronous error-handling thread is switched off
    (TORCH_NCCL_ASYNC_ERROR_HANDLING=0).  Eager multi-GPU training keeps PyTorch's default: a failed or hung
    collective on one rank aborts the job instead of hanging it."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        if backend is None:
            # PARADIS_DIST_BACKEND=gloo lets a 1-GPU box exercise the N>1 code path (tests only)
            backend = os.environ.get("PARADIS_DIST_BACKEND") or \
                ("nccl" if torch.cuda.is_available() else "gloo")
        if backend == "nccl":
            torch.cuda.set_device(local)
            if capturable:
                os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "0")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local, world


def wrap_ddp(model, *, bucket_cap_mb: float = 32, device_ids: Optional[Sequence[int]] = None,
             static_graph: bool = False, force: bool = False, capturable: bool = False):
    """Batch-sharded data parallelism (the reference's only strategy, ``train.py:49``): full replica
    per GPU, bucketed gradient all-reduce (RCCL over xGMI) overlapped with backward.  Geometry
    buffers are deterministic functions of the grid, so buffer broadcast is disabled; the graph is
    static, gradients alias the buckets.

    ``force``: wrap even in a one-rank process group (a world_size = 1 ``nccl`` group initialises RCCL and runs
    its all-reduce kernels: the one-GPU stand-in for the N > 1 path, tests/test_hip_ddp.py and the ``ddp_overhead_ms``
    leg of bench.py).  ``capturable``: construct the wrapper on a side stream, which is what capturing a DDP step
    into a HIP graph requires (``GraphedTrainStep``; the Reducer's bucket views and streams must not belong to the
    capturing stream)."""
    if not dist.is_initialized() or (dist.get_world_size() == 1 and not force):
        return model

    def build():
        return torch.nn.parallel.DistributedDataParallel(
            model, device_ids=list(device_ids) if device_ids is not None else None,
            broadcast_buffers=False, gradient_as_bucket_view=True, bucket_cap_mb=bucket_cap_mb,
            static_graph=bool(static_graph))
    if capturable and torch.cuda.is_available():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ddp = build()
        torch.cuda.current_stream().wait_stream(side)
        return ddp
    return build()


def max_over_ranks(value: float, device) -> float:
    if not dist.is_initialized() or dist.get_world_size() == 1:
        return value
    t = torch.tensor([value], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def barrier():
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.barrier()
