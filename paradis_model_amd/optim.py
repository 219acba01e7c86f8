"""AdamW step on the HIP device (reference ``trainer.py:327-335`` uses
``torch.optim.AdamW(params, lr, weight_decay, betas)``).  Same update rule and operation order as
``torch.optim.AdamW`` (decoupled weight decay, bias-corrected moments, eps added after the sqrt);
state-dict layout compatible with it (``step``, ``exp_avg``, ``exp_avg_sq``)."""
import ctypes

import torch

from . import ops
from ._lib import check, dptr, lib, require_hip, stream_ptr
from ._tables import AddressTable, chunk_list


class AdamW(torch.optim.Optimizer):
    """``capturable=True``: the step count and the learning rate of every group also live on the device
    (``paradis_adamw_multi_d(..., dev_state)``), so a HIP graph captured around ``step()`` stays valid from replay to
    replay (``harness.GraphedTrainStep``); same formula, the bias corrections formed in double on the device (agrees with the
    host-side path to ~1 ulp of the fp32 corrections: the device pow is not the host libm, test bound 1e-6).

    The learning rate of a capturable optimiser changes in one of two ways: the host sets ``group["lr"]`` and calls
    ``sync_device_state()`` (a blocking copy: fine per epoch, a queue drain when done per step), or a
    ``schedule.DeviceSchedule`` is attached (``attach_schedule``) and one launch inside ``step()`` - behind the ticks of the
    groups' step counts, in front of their updates - writes every group's learning rate for its step from a device table;
    ``group["lr"]`` then mirrors the table."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, capturable=False):
        if lr < 0 or eps < 0 or weight_decay < 0 or not 0 <= betas[0] < 1 or not 0 <= betas[1] < 1:
            raise ValueError("invalid AdamW hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.capturable = bool(capturable)
        # keyed, like the pointer-table caches, by the group's index in the FULL ``param_groups`` (a subclass that
        # updates only some groups by this class's kernels must not renumber them: sync_device_state walks the full list)
        self._dev_state = {}      # group index -> [int32[2] device tensor, lr it holds]
        self._schedule = None

    def attach_schedule(self, schedule) -> None:
        """``schedule``: a ``schedule.DeviceSchedule`` built on this optimiser (``None`` detaches)"""
        if schedule is not None and not self.capturable:
            raise ValueError("a device schedule needs a capturable optimiser (the learning rate must live on the device)")
        self._schedule = schedule

    def _device_state(self, gi, group, dev, step_before):
        """int32[2] = [step count, bits of lr] of group ``gi`` on the device (created at the group's first update)"""
        import struct
        ent = self._dev_state.get(gi)
        lr_bits = struct.unpack("<i", struct.pack("<f", float(group["lr"])))[0]
        if ent is None:
            ent = [torch.tensor([step_before, lr_bits], dtype=torch.int32, device=dev), float(group["lr"])]
            self._dev_state[gi] = ent
        elif ent[1] != float(group["lr"]):
            if self._schedule is not None:
                ent[1] = float(group["lr"])      # the schedule launch writes it on the device
                return ent[0]
            if ent[0].is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("AdamW(capturable): the learning rate changed inside a graph capture")
            ent[0][1:2].copy_(torch.tensor([lr_bits], dtype=torch.int32), non_blocking=False)
            ent[1] = float(group["lr"])
        return ent[0]

    def sync_device_state(self):
        """push the host-side learning rates to the device (call between graph replays after a scheduler step)"""
        for gi, group in enumerate(self.param_groups):
            if gi in self._dev_state:
                self._device_state(gi, group, self._dev_state[gi][0].device, 0)

    def _group_step(self, group):
        """the step count of the group's parameters that have state (``None``: none has)"""
        for p in group["params"]:
            st = self.state.get(p)
            if st:
                return int(st["step"])
        return None

    def note_replayed(self):
        """a captured step() was replayed: advance the host-side step counts (state_dict compatibility) and, under a
        device schedule, set ``group["lr"]`` to what the replay used"""
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                st = self.state.get(p)
                if st:
                    st["step"] += 1
            if self._schedule is not None:
                self._mirror_lr(gi, group, self._group_step(group))

    def _mirror_lr(self, gi, group, step):
        if step is not None and step >= 1:
            lr = self._schedule.host_lr(gi, step - 1)
            group["lr"] = lr
            if gi in self._dev_state:
                self._dev_state[gi][1] = lr

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plans = [pl for pl in (self._prepare_group(gi, g) for gi, g in enumerate(self.param_groups)) if pl is not None]
        self._run(plans)
        return loss

    def _run(self, plans):
        """``plans``: what ``_prepare_group`` returned for the groups that have gradients.  Capturable: first every
        group's device step count is advanced and (with a schedule) its learning rate written, then the updates run."""
        if self.capturable:
            for pl in plans:
                gi, group = pl["gi"], pl["group"]
                if pl["step"] is None:
                    raise RuntimeError("AdamW(capturable) needs contiguous parameters with one common step count per group")
                if self._schedule is not None:
                    self._mirror_lr(gi, group, pl["step"])
                pl["dev_state"] = self._device_state(gi, group, pl["params"][0].device, pl["step"] - 1)
                check(lib.paradis_adamw_tick(dptr(pl["dev_state"]), stream_ptr()), "adamw_tick")
            if self._schedule is not None and plans:
                self._schedule.apply()
        for pl in plans:
            self._update_group(pl)
        ops.weights_updated()     # the kernels write through raw pointers: no version-counter bump

    def _prepare_group(self, gi, group):
        """host bookkeeping of one group's update: state creation, step counts.  ``step``: the common step count when
        the group can go through the fused launch, else ``None``."""
        params = [p for p in group["params"] if p.grad is not None]
        if not params:
            return None
        steps = set()
        for p in params:
            require_hip(p, p.grad)
            state = self.state[p]
            if not state:
                state["step"] = 0
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["step"] += 1
            steps.add(int(state["step"]))
        uniform = len(steps) == 1 and all(p.is_contiguous() and p.grad.is_contiguous() for p in params)
        return dict(gi=gi, group=group, params=params, step=steps.pop() if uniform else None, dev_state=None)

    def _update_group(self, pl):
        group, params = pl["group"], pl["params"]
        st = stream_ptr()
        if pl["step"] is not None and (len(params) > 1 or self.capturable):
            self._step_group_fused(pl["gi"], group, params, pl["step"], st, pl["dev_state"])
            return
        b1, b2 = group["betas"]
        for p in params:
            state = self.state[p]
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            check(lib.paradis_adamw_step_d(dptr(p), dptr(g), dptr(state["exp_avg"]),
                                         dptr(state["exp_avg_sq"]), p.numel(), group["lr"], b1, b2,
                                         group["eps"], group["weight_decay"], int(state["step"]), st),
                  "adamw_step")

    def _pointer_caches(self):
        for name in ("_fused_cache", "_muon_cache"):
            for gi, c in self.__dict__.get(name, {}).items():
                yield (name, gi), c

    def snapshot_pointer_tables(self):
        """copies of the pinned address tables of the fused groups and of the Muon-family matrix groups
        (``harness.GraphedTrainStep``: a captured step re-reads them on every replay)"""
        return {key: c["addr"].snapshot() for key, c in self._pointer_caches()}

    def restore_pointer_tables(self, tables) -> None:
        caches = dict(self._pointer_caches())
        for key, t in tables.items():
            c = caches.get(key)
            if c is not None:
                c["addr"].restore(t)

    def _step_group_fused(self, gi, group, params, step, st, dev_state=None):
        """One launch for the group (``paradis_adamw_multi_d``).  Only the chunk list (a function of the
        parameter sizes) is cached; the four address rows (parameter, gradient, both moments) are
        rewritten every step (``_tables.AddressTable``)."""
        dev = params[0].device
        key = tuple((id(p), p.numel()) for p in params) + (str(dev),)
        cache = self.__dict__.setdefault("_fused_cache", {})
        c = cache.get(gi)
        if c is None or c["key"] != key:
            T = len(params)
            ct, co = chunk_list([p.numel() for p in params], lib.paradis_adamw_chunk())
            c = cache[gi] = dict(
                key=key, T=T, addr=AddressTable(4, T, dev),
                numel=torch.tensor([p.numel() for p in params], dtype=torch.int64, device=dev),
                chunk_tensor=torch.tensor(ct, dtype=torch.int32, device=dev),
                chunk_off=torch.tensor(co, dtype=torch.int64, device=dev), n_chunks=len(ct))
        T = c["T"]
        moments = [(self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in params]
        for m, v in moments:
            require_hip(m, v)
            if not (m.is_contiguous() and v.is_contiguous()):
                raise RuntimeError("AdamW: non-contiguous optimizer state")
        c["addr"].write([p.data_ptr() for p in params] + [p.grad.data_ptr() for p in params]
                        + [m.data_ptr() for m, _ in moments] + [v.data_ptr() for _, v in moments])
        b1, b2 = group["betas"]
        check(lib.paradis_adamw_multi_d(dptr(c["addr"].ptrs), dptr(c["numel"]), dptr(c["chunk_tensor"]),
                                      dptr(c["chunk_off"]), T, c["n_chunks"], group["lr"], b1, b2, group["eps"],
                                      group["weight_decay"], step, dptr(dev_state), st), "adamw_multi")


# ---------------------------------------------------------------------------------------------
# Muon / NorMuon (the reference's default optimiser family, trainer.py:337-364, from `dion`)
# ---------------------------------------------------------------------------------------------
def build_param_groups(model, lr, weight_decay, optimizer_name):
    """The reference's split of the parameters between the two algorithms (rule of reference
    ``trainer.py:24-64``): a ``weight`` owned directly by a Linear / ConvNd module is a matrix for the
    Muon family (conv kernels flattened to 2-D); every other trainable parameter - the biases of those
    modules first, then norm scales, GlobalBias factors, gates - is updated by AdamW.  Group order and
    the order inside each group follow module traversal, so optimiser state dicts index parameters
    the way the reference's do."""
    from torch import nn
    matrix_owner = (nn.Linear, nn.Conv1d, nn.Conv2d, nn.Conv3d)
    role = {}                                  # id(parameter) -> "matrix" | "bias": first owner wins
    for module in model.modules():
        if isinstance(module, matrix_owner):
            for name, kind in (("weight", "matrix"), ("bias", "bias")):
                p = module._parameters.get(name)
                if p is not None:
                    role.setdefault(id(p), kind)
    buckets = {"matrix": [], "bias": [], None: []}
    for p in model.parameters():               # de-duplicated, module traversal order
        if p.requires_grad:
            buckets[role.get(id(p))].append(p)
    return [dict(params=buckets["matrix"], algorithm=optimizer_name, lr=lr, weight_decay=weight_decay,
                 flatten=True),
            dict(params=buckets["bias"] + buckets[None], algorithm="adamw", lr=lr, weight_decay=weight_decay)]


def _adjusted_lr(lr, shape, adjust):
    import math
    fan_out, fan_in = shape[0], math.prod(shape[1:])
    if adjust is None:
        return lr
    if adjust == "spectral_norm":
        return lr * math.sqrt(fan_out / fan_in)
    if adjust == "rms_norm":
        return lr * 0.2 * math.sqrt(max(fan_out, fan_in))
    raise ValueError(f"unknown adjust_lr {adjust!r}")


def _lr_scale(shape, adjust):
    """``_adjusted_lr(lr, shape, adjust) / lr``: what ``paradis_muon_step_d`` multiplies the device-side lr by"""
    import math
    fan_out, fan_in = shape[0], math.prod(shape[1:])
    if adjust is None:
        return 1.0
    if adjust == "spectral_norm":
        return math.sqrt(fan_out / fan_in)
    if adjust == "rms_norm":
        return 0.2 * math.sqrt(max(fan_out, fan_in))
    raise ValueError(f"unknown adjust_lr {adjust!r}")


class Muon(AdamW):
    """Muon with the constructor of ``dion.Muon`` as the reference calls it (trainer.py:347-354):
    parameter groups carry ``algorithm`` ("muon" / "normuon" for 2-D-flattened weights, "adamw" for
    the rest, see ``build_param_groups``).  The matrix update runs in one C-ABI call per weight
    (``paradis_muon_step``: fp32 Newton-Schulz on the GEMMs of ``ops`` - bf16x3 split unless ``ops.GEMM_SCHEME`` is exact - no Triton); AdamW groups use the fused kernel
    of the base class.  ``dion`` is neither vendored nor pinned by the reference: the algorithm is
    restated from its published form (oracle/muon_oracle.py), parity unpinned."""

    _NORMUON = False
    _DEFAULT_ADJUST = "spectral_norm"

    def __init__(self, params, lr=0.01, mu=0.95, betas=(0.9, 0.95), weight_decay=0.01, epsilon=1e-8,
                 nesterov=False, adjust_lr="default", flatten=False, use_triton=False, muon_beta2=0.95,
                 capturable=False):
        del use_triton   # accepted for signature compatibility; there is no Triton on this path
        if adjust_lr == "default":
            adjust_lr = self._DEFAULT_ADJUST
        params = list(params)
        if params and not isinstance(params[0], dict):
            params = [dict(params=params, algorithm="normuon" if self._NORMUON else "muon")]
        for gdict in params:
            gdict.setdefault("algorithm", "normuon" if self._NORMUON else "muon")
        super().__init__(params, lr=lr, betas=betas, eps=epsilon, weight_decay=weight_decay, capturable=capturable)
        for group in self.param_groups:
            group.setdefault("mu", mu)
            group.setdefault("nesterov", nesterov)
            group.setdefault("adjust_lr", adjust_lr)
            group.setdefault("flatten", flatten)
            group.setdefault("muon_beta2", muon_beta2)

    @torch.no_grad()
    def step(self, closure=None):
        """the matrix groups first, then the AdamW groups; every group keeps its index in ``param_groups`` (the key of
        its device state and of its pinned address table)"""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        indexed = list(enumerate(self.param_groups))
        for _, group in indexed:
            if group["algorithm"] not in ("muon", "normuon", "adamw"):
                raise ValueError(f"unknown algorithm {group['algorithm']!r}")
        plans = [self._prepare_matrix_group(gi, g) for gi, g in indexed if g["algorithm"] != "adamw"]
        plans += [self._prepare_group(gi, g) for gi, g in indexed if g["algorithm"] == "adamw"]
        self._run([pl for pl in plans if pl is not None])
        return loss

    def _update_group(self, pl):
        if pl.get("matrix"):
            self._step_matrix_group(pl)
        else:
            AdamW._update_group(self, pl)

    def _prepare_matrix_group(self, gi, group):
        normuon = group["algorithm"] == "normuon"
        params = [p for p in group["params"] if p.grad is not None]
        if not params:
            return None
        steps = set()
        for p in params:
            require_hip(p, p.grad)
            if p.dim() < 2:
                raise ValueError("Muon parameters must be matrices (use an adamw group for the rest)")
            if p.dim() > 2 and not group["flatten"]:
                raise ValueError("conv weights need flatten=True (reference trainer.py:54)")
            if not p.is_contiguous():
                raise ValueError("Muon: non-contiguous parameter")
            state = self.state[p]
            if not state:
                state["step"] = 0
                state["momentum"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if normuon:
                    state["variance_neuron"] = torch.zeros(p.shape[0], 1, dtype=p.dtype, device=p.device)
            state["step"] += 1
            steps.add(int(state["step"]))
        return dict(gi=gi, group=group, params=params, step=steps.pop() if len(steps) == 1 else None, dev_state=None,
                    matrix=True)

    def _step_matrix_group(self, pl):
        """Same-shaped matrices are updated together (one ``paradis_muon_step`` per shape: the batched
        Newton-Schulz GEMMs fill the chip).  One device table of the w / g / momentum / variance
        addresses serves all shapes; all four rows are rewritten each step (``_tables.AddressTable``: state tensors
        can be replaced by ``load_state_dict`` behind the same parameter ids).  Capturable: the learning rate is read from the group's device
        state (``paradis_muon_step_d``), and inside a graph capture the table copy is a graph node, as in
        ``_step_group_fused``."""
        gi, group, params = pl["gi"], pl["group"], pl["params"]
        normuon = group["algorithm"] == "normuon"
        dev = params[0].device
        key = tuple((id(p), tuple(p.shape)) for p in params) + (str(dev), normuon)
        cache = self.__dict__.setdefault("_muon_cache", {})
        c = cache.get(gi)
        if c is None or c["key"] != key:
            by_shape = {}
            for p in params:
                by_shape.setdefault((p.shape[0], p.numel() // p.shape[0], tuple(p.shape)), []).append(p)
            order, shapes = [], []
            for (rows, cols, full), ps in by_shape.items():
                shapes.append((rows, cols, full, len(order), len(ps)))
                order.extend(ps)
            T = len(order)
            ws_bytes = max(lib.paradis_muon_ws_bytes(n, rows, cols) for rows, cols, _, _, n in shapes)
            c = cache[gi] = dict(key=key, order=order, shapes=shapes, T=T, addr=AddressTable(4, T, dev),
                                 ws=torch.empty(ws_bytes // 4 + 64, dtype=torch.float32, device=dev))
        T = c["T"]
        grads = []
        for p in c["order"]:
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            grads.append(g)          # keep alive until the kernels are queued
        mom = [self.state[p]["momentum"] for p in c["order"]]
        var = [self.state[p]["variance_neuron"] for p in c["order"]] if normuon else []
        require_hip(*mom, *var)
        if c["addr"].write([p.data_ptr() for p in c["order"]] + [g.data_ptr() for g in grads]
                           + [m.data_ptr() for m in mom] + ([v.data_ptr() for v in var] if normuon else [0] * T)):
            c["captured_grads"] = grads      # every replay reads them at these addresses: they live as long as the table
        st = stream_ptr()
        lr = group["lr"]
        base = c["addr"].ptrs.data_ptr()
        split = 1 if ops.GEMM_SCHEME != ops.GEMM_EXACT else 0
        for rows, cols, full, off, n in c["shapes"]:
            if self.capturable:
                check(lib.paradis_muon_step_d(ctypes.c_void_p(base + 8 * off), T, n, rows, cols, lr,
                                              _adjusted_lr(lr, full, group["adjust_lr"]), group["mu"],
                                              group["muon_beta2"], group["weight_decay"], group["eps"],
                                              int(bool(group["nesterov"])), int(normuon), split, dptr(c["ws"]),
                                              dptr(pl["dev_state"]), _lr_scale(full, group["adjust_lr"]), st),
                      "muon_step")
                continue
            check(lib.paradis_muon_step(ctypes.c_void_p(base + 8 * off), T, n, rows, cols, lr,
                                        _adjusted_lr(lr, full, group["adjust_lr"]), group["mu"],
                                        group["muon_beta2"], group["weight_decay"], group["eps"],
                                        int(bool(group["nesterov"])), int(normuon), split, dptr(c["ws"]), st),
                  "muon_step")


class NorMuon(Muon):
    """``dion.NorMuon`` as called at reference trainer.py:355-362 (the shipped default,
    config/paradis_settings.yaml:117): Muon + per-neuron second-moment normalisation."""

    _NORMUON = True
    _DEFAULT_ADJUST = "rms_norm"
