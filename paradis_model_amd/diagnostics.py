"""Training diagnostics: what the reference's ``LitParadis`` logs on every optimiser step when
``training.log_additional_stats`` is on - the gradient statistics per parameter group of ``on_before_optimizer_step``
(reference ``trainer.py:844-923``), the per-channel training losses as the mean over the rollout steps
(``trainer.py:520-556, 591-617``) and the training loss.

The reference composes the gradient statistics from ATen calls per parameter: up to four squares or products, four full
reductions and four scalar adds for each of the 335 tensors of the default model.  Here one HIP launch pair
(``csrc/stats.hip``) reads every parameter, gradient and first moment once and leaves a dense row per group on the device;
the per-channel losses come from the validation score kernel (``validate.score``).  Nothing waits for the device until
``TrainStats.result``, which makes one device-to-host read.

No CPU fallback: the tensors must live on the HIP device (the CPU restatement for the tests is tests/stats_oracle.py).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import _lib
from ._lib import dptr, require_hip, stream_ptr
from ._tables import AddressTable, chunk_list

COLS = 8                                    # Sp2, Sg2, Sgm, Sm2, grad norm, gradratio, pnorm, alignment
SUM_P2, SUM_G2, SUM_GM, SUM_M2, GRAD, RATIO, PNORM, ALIGN = range(COLS)
_PREFIXES = ("module.", "_orig_mod.")       # DistributedDataParallel / torch.compile wrappers


def group_key(name: str) -> str:
    """first component of a parameter name relative to the ``Paradis`` module: the reference's ``name.split(".")[1]`` on
    ``LitParadis`` (whose model attribute adds one leading component)"""
    stripped = True
    while stripped:
        stripped = False
        for pre in _PREFIXES:
            if name.startswith(pre):
                name, stripped = name[len(pre):], True
    return name.split(".")[0]


def chunk_table(numels: Sequence[int], groups: Sequence[int], n_groups: int, chunk: int):
    """(chunk_tensor, chunk_off, group_first_chunk [n_groups + 1]) as Python lists: one chunk per ``chunk`` elements of
    every tensor, sorted by group (then tensor, then offset), so that a group's chunks are contiguous"""
    if len(numels) != len(groups):
        raise ValueError("chunk_table: one group index per tensor")
    if any(not 0 <= int(g) < n_groups for g in groups):
        raise ValueError("chunk_table: group index out of range")
    ct: List[int] = []
    co: List[int] = []
    first = [0] * (n_groups + 1)
    for g in range(n_groups):
        first[g] = len(ct)
        gt, go = chunk_list(numels, chunk, [t for t, tg in enumerate(groups) if tg == g])
        ct += gt
        co += go
    first[n_groups] = len(ct)
    return ct, co, first


class StatsPlan:
    """Device tables of ``paradis_param_stats`` for one list of tensor sizes and group indices (they depend on nothing
    else), the pinned staging buffer of the three address rows, the workspace and - unless ``out`` is given - the
    result rows ``[n_groups + 1, 8]``."""

    def __init__(self, numels: Sequence[int], groups: Sequence[int], n_groups: int, device, out=None):
        self.T, self.G = len(numels), int(n_groups)
        chunk = _lib.lib.paradis_param_stats_chunk()
        ct, co, first = chunk_table(numels, groups, self.G, chunk)
        self.n_chunks = len(ct)
        self.addr = AddressTable(3, self.T, device)
        with torch.inference_mode(False):
            self.numel = torch.tensor(list(numels) or [0], dtype=torch.int64, device=device)
            self.chunk_tensor = torch.tensor(ct or [0], dtype=torch.int32, device=device)
            self.chunk_off = torch.tensor(co or [0], dtype=torch.int64, device=device)
            self.group_first = torch.tensor(first, dtype=torch.int32, device=device)
            ws = int(_lib.lib.paradis_param_stats_ws_bytes(self.n_chunks))
            self.ws = torch.empty(max(1, ws // 8), dtype=torch.float64, device=device)
            self.out = out if out is not None else torch.zeros(self.G + 1, COLS, device=device)
        if self.out.numel() != (self.G + 1) * COLS or not self.out.is_contiguous():
            raise ValueError(f"param_stats: out must be a dense [{self.G + 1}, {COLS}] tensor")
        require_hip(self.out)

    def launch(self, params, grads, moments) -> torch.Tensor:
        """rewrite the address rows (pinned staging buffer, non-blocking copy) and run the launch pair on the current stream"""
        T = self.T
        if not (len(params) == len(grads) == len(moments) == T):
            raise ValueError(f"param_stats: the plan was built for {T} tensors")
        addr = [0] * (3 * T)
        nbytes = 0
        for t, (p, g, m) in enumerate(zip(params, grads, moments)):
            require_hip(p, g, m)
            for x, what in ((p, "parameter"), (g, "gradient"), (m, "moment")):
                if x is None:
                    continue
                if not x.is_contiguous():
                    raise RuntimeError(f"param_stats: non-contiguous {what}")
                if x.numel() != p.numel():
                    raise ValueError(f"param_stats: a {what} of {x.numel()} elements for a parameter of {p.numel()}")
            addr[t] = p.data_ptr()
            addr[T + t] = g.data_ptr() if g is not None else 0
            addr[2 * T + t] = m.data_ptr() if (m is not None and g is not None) else 0
            nbytes += 4 * p.numel() * (1 + (g is not None) + (g is not None and m is not None))
        self.addr.write(addr)
        _lib.call("param_stats", float(nbytes), dptr(self.addr.ptrs), dptr(self.numel), dptr(self.chunk_tensor),
                  dptr(self.chunk_off), dptr(self.group_first), T, self.n_chunks, self.G, dptr(self.ws), dptr(self.out),
                  stream_ptr())
        return self.out

    def snapshot_pointer_tables(self):
        return self.addr.snapshot()

    def restore_pointer_tables(self, table) -> None:
        self.addr.restore(table)


def param_stats(params, grads, moments, groups: Sequence[int], n_groups: Optional[int] = None,
                plan: Optional[StatsPlan] = None) -> torch.Tensor:
    """``[n_groups + 1, 8]`` fp32 on the device by ``paradis_param_stats``: per group ``{sum p^2, sum g^2, sum g.m,
    sum m^2, grad norm, gradratio, pnorm, alignment}``, last row the totals (include/paradis_hip.h).

    params: dense fp32 device tensors; grads / moments: the same length, entries may be ``None`` (a moment without a
    gradient is ignored, as the reference ignores it); groups: the group index of every tensor.  A non-contiguous
    tensor raises.  ``plan``: a ``StatsPlan`` of the same sizes and groups to reuse (its ``out`` is returned, overwritten
    by the next call); without it the tables are built for this call.  No host synchronisation with a plan."""
    params = list(params)
    if plan is None:
        if not params:
            raise ValueError("param_stats: no tensors")
        G = int(n_groups) if n_groups is not None else (max(groups) + 1)
        require_hip(*params)
        plan = StatsPlan([p.numel() for p in params], list(groups), G, params[0].device)
    return plan.launch(params, list(grads), list(moments))


class TrainStats:
    """The ``log_additional_stats`` diagnostics of one training step (module docstring).

    Groups: the key of a parameter is the first component of its name relative to the ``Paradis`` module (a DDP
    ``module.`` and a compile ``_orig_mod.`` prefix stripped), groups ordered by sorted key.

    ``before_optimizer_step(optimizer)``: for every parameter ``p``, ``p.grad`` and ``optimizer.state[p]["exp_avg"]``
    where that key exists (the literal key: Muon / NorMuon matrices keep ``"momentum"`` and have no alignment, the
    reference's behaviour with ``dion``; on the first step there is no state yet) go through ``paradis_param_stats``.
    ``on_rollout_step(out, target)``: the per-channel losses of one rollout step (``validate.score``) into a device
    row.  ``record_loss(loss)``: the step loss.  ``harness.TrainStep(..., stats=...)`` calls all of them; inside a
    HIP-graph capture every launch and the address-table copy are graph nodes.

    ``result(sync_dist=False)``: one device-to-host read; the reference's keys ``grad/total``, ``grad/<k>``,
    ``gradratio/<k>``, ``pnorm/<k>`` for every group with at least one gradient, ``grad_alignment/<k>`` /
    ``grad_alignment/total`` where the sum of squared moments is positive, ``train_loss_channel_weighted/<name>``,
    ``train_loss_channel_unweighted/<name>`` (means over the rollout steps; zeros for an ``"amse"`` loss, as in the
    validator) and ``train_loss`` - the real step loss (the reference logs 0 here: INTEGRATION.md)."""

    def __init__(self, model, loss_fn, *, channel_losses: bool = True):
        self.model, self.loss_fn = model, loss_fn
        self.channel_losses = bool(channel_losses)
        self.channel_names = list(loss_fn.output_name_order) if self.channel_losses else []
        self.named = [(n, p) for n, p in model.named_parameters() if p is not None]
        keys = [group_key(n) for n, _ in self.named]
        self.group_keys = sorted(set(keys))
        self.groups = [self.group_keys.index(k) for k in keys]
        self._plan: Optional[StatsPlan] = None
        self._key = None
        self._vec = None            # device fp32: [(G + 1) * 8 stats | C weighted | C unweighted | loss]
        self._rows: List[torch.Tensor] = []
        self._s = 0                 # rollout steps scored since begin_step()
        self._reported: List[bool] = []
        self._have = {"stats": False, "loss": False, "chan": False}

    # ------------------------------------------------------------------ layout of the metric vector
    @property
    def _n_stats(self) -> int:
        return (len(self.group_keys) + 1) * COLS

    def _vector(self, device) -> torch.Tensor:
        n = self._n_stats + 2 * len(self.channel_names) + 1
        if self._vec is None or self._vec.device != device or self._vec.numel() != n:
            with torch.inference_mode(False):
                self._vec = torch.zeros(n, device=device)
            self._plan = None
        return self._vec

    # ------------------------------------------------------------------ hooks of the training step
    def begin_step(self) -> None:
        self._s = 0

    @torch.no_grad()
    def on_rollout_step(self, out: torch.Tensor, target: torch.Tensor) -> None:
        if not self.channel_losses:
            return
        from . import validate
        require_hip(out, any_dtype=True)
        pred = out.detach()
        if pred.dtype != torch.float32:
            pred = pred.float()
        C = pred.shape[1]
        if self._s >= len(self._rows) or self._rows[self._s].device != pred.device:
            with torch.inference_mode(False):
                row = torch.zeros(validate.row_size(C, 0), device=pred.device)
            self._rows[self._s:self._s + 1] = [row]
        validate.score(pred, target, self.loss_fn, None, self._rows[self._s])
        self._s += 1

    @torch.no_grad()
    def before_optimizer_step(self, optimizer) -> None:
        params = [p for _, p in self.named]
        if not params:
            raise RuntimeError("TrainStats: the model has no parameters")
        grads = [p.grad for p in params]
        moments = []
        for p in params:
            st = optimizer.state.get(p) if p.grad is not None else None
            moments.append(st["exp_avg"] if st and "exp_avg" in st else None)
        dev = params[0].device
        require_hip(*params)
        vec = self._vector(dev)
        key = tuple((id(p), p.numel()) for p in params) + (str(dev),)
        if self._plan is None or self._key != key:
            G = len(self.group_keys)
            self._plan = StatsPlan([p.numel() for p in params], self.groups, G, dev,
                                   out=vec[:self._n_stats].view(G + 1, COLS))
            self._key = key
        self._plan.launch(params, grads, moments)
        self._reported = [False] * len(self.group_keys)
        for gi, g in zip(self.groups, grads):
            if g is not None:
                self._reported[gi] = True
        self._have["stats"] = True
        if self.channel_losses and self._s > 0:
            C = len(self.channel_names)
            mean = torch.stack(self._rows[:self._s]).mean(dim=0)
            vec[self._n_stats:self._n_stats + 2 * C].copy_(mean[1:1 + 2 * C])
            self._have["chan"] = True

    @torch.no_grad()
    def record_loss(self, loss: torch.Tensor) -> None:
        require_hip(loss)
        vec = self._vector(loss.device)
        vec[-1:].copy_(loss.detach().reshape(1))
        self._have["loss"] = True

    # ------------------------------------------------------------------ the pinned address table and HIP graphs
    def snapshot_pointer_tables(self):
        """a copy of the pinned address table (``harness.GraphedTrainStep``: the captured copy node re-reads it on every
        replay)"""
        return None if self._plan is None else self._plan.snapshot_pointer_tables()

    def restore_pointer_tables(self, table) -> None:
        if self._plan is not None:
            self._plan.restore_pointer_tables(table)

    # ------------------------------------------------------------------ the logged values
    def result(self, sync_dist: bool = False) -> Dict[str, float]:
        if self._vec is None or not self._have["stats"]:
            raise RuntimeError("TrainStats.result: before_optimizer_step has not run")
        import torch.distributed as dist
        vec = self._vec
        if sync_dist and dist.is_available() and dist.is_initialized():
            vec = vec.double()
            if dist.get_backend() == "gloo":
                vec = vec.cpu()              # the one device-to-host read, in front of the host-side sum
            dist.all_reduce(vec, op=dist.ReduceOp.SUM)
            vec = vec.cpu() / dist.get_world_size()
        else:
            vec = vec.cpu().double()
        v = vec.tolist()
        G = len(self.group_keys)
        res = {"grad/total": v[G * COLS + GRAD]}
        for gi, k in enumerate(self.group_keys):
            if not self._reported[gi]:
                continue
            row = v[gi * COLS:(gi + 1) * COLS]
            res[f"grad/{k}"] = row[GRAD]
            res[f"gradratio/{k}"] = row[RATIO]
            res[f"pnorm/{k}"] = row[PNORM]
            if row[SUM_M2] > 0:
                res[f"grad_alignment/{k}"] = row[ALIGN]
        if v[G * COLS + SUM_M2] > 0:
            res["grad_alignment/total"] = v[G * COLS + ALIGN]
        if self._have["chan"]:
            C = len(self.channel_names)
            for c, name in enumerate(self.channel_names):
                res[f"train_loss_channel_weighted/{name}"] = v[self._n_stats + c]
                res[f"train_loss_channel_unweighted/{name}"] = v[self._n_stats + C + c]
        if self._have["loss"]:
            res["train_loss"] = v[-1]
        return res
