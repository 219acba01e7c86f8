"""What the no-grad loops share: the autoregressive step of ``forecast.Forecaster.run`` and ``validate.Validator.step``
(``Stepper``: with ``graph=True`` one HIP-graph replay) and the two-slot hand-over of finished chunks from the device
to pinned host memory through a side stream (``ChunkRing``).  No CPU fallback: the tensors must live on the HIP device."""
from types import SimpleNamespace

import torch

from . import harness


class GraphedStep:
    """input assembly + model + feedback copy into the static input, captured once per (B, H, W)"""

    def __init__(self, model, inp, forc, const, num_common, n_inputs):
        with torch.inference_mode(False), torch.no_grad():
            self.inp, self.forc, self.const = (torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t)
                                               for t in (inp, forc, const))      # dense, whatever the views' strides

            def step():
                mi = harness.assemble_model_input(self.inp.unsqueeze(1), self.forc.unsqueeze(1), self.const.unsqueeze(1))
                y = model(mi)
                self.inp.copy_(harness.next_input(mi, y, num_common, n_inputs))
                return y
            self.graph, self.out = harness.capture_forward(step)

    def __call__(self, forc_step):
        self.forc.copy_(forc_step, non_blocking=True)
        self.graph.replay()
        return self.out


class Stepper:
    """The autoregressive no-grad step (reference trainer.py:534-538,710-729).  ``begin(input_data [B,1,n_inputs*
    num_common,H,W], forcings [B,S,H,W,F], constants [B,1,H,W,K])``; ``step(s)``, s = 0, 1, ...: the output of ``forward``
    on (current input, forcings of step s, constants), fed back into the input; ``end()`` lets go of the batch.
    ``graph=True``: a step is one forcing copy and one replay of a ``GraphedStep``, captured once per (B, H, W) (``steps``)
    outside ``ops.frozen_weights()`` - the weight-image kernels are nodes of the graph, so parameters written in place
    between runs are honoured by the next replay; the output is a static tensor that the next step overwrites."""

    def __init__(self, forward, num_common: int, n_inputs: int, graph: bool):
        self.forward, self.num_common, self.n_inputs, self.graph = forward, int(num_common), int(n_inputs), bool(graph)
        self.steps = {}            # (B, H, W) -> GraphedStep
        self.end()

    def end(self) -> None:
        self._forc = self._const = self._cur = self._fn = None

    def begin(self, input_data, forcings, constants) -> None:
        self._const = constants[:, :1].permute(0, 1, 4, 2, 3)
        self._forc = forcings.permute(0, 1, 4, 2, 3)
        self._cur, self._fn = input_data, None
        if self.graph:
            key = (input_data.shape[0], *input_data.shape[-2:])         # (B, H, W)
            if key not in self.steps:
                from . import ops
                with ops.frozen_weights(False):
                    self.steps[key] = GraphedStep(self.forward, input_data[:, 0], self._forc[:, 0], self._const[:, 0],
                                                  self.num_common, self.n_inputs)
            self._fn = self.steps[key]
            self._fn.inp.copy_(input_data[:, 0], non_blocking=True)
            self._fn.const.copy_(self._const[:, 0], non_blocking=True)

    def step(self, s: int) -> torch.Tensor:
        if self._fn is not None:
            return self._fn(self._forc[:, s])
        mi = harness.assemble_model_input(self._cur, self._forc[:, s].unsqueeze(1), self._const)
        out = self.forward(mi)
        self._cur = harness.next_input(mi, out, self.num_common, self.n_inputs).unsqueeze(1)
        return out


def _chunk(t, n):
    """the leading ``n`` states per sample of ``t``'s storage ``[B, N, ...]`` as a dense ``[B, n, ...]`` tensor"""
    return t.view(-1)[:t.numel() // t.shape[1] * n].view(t.shape[0], n, *t.shape[2:])


class ChunkRing:
    """Two slots that take turns between the stream that fills a chunk and a side stream that copies it to the host.
    ``shapes``: name -> ``(B, n, ...)``, the full shape of a named (device tensor, pinned tensor) pair; a slot holds each
    pair (pinned from ``pin()`` on), a ``filled`` and a ``copied`` event and a used flag; the ring one side stream and
    ``pending``, the chunks enqueued for the copy and not yet delivered.  The contract, for chunk ``i`` of ``n`` states,
    which ``open`` puts into slot ``k = i & 1``, main = the current stream:

    1. ``open(n)``, before the main stream first writes slot ``k`` for a new chunk, waits on ``copied[k]`` if the slot
       has been used, and returns the device views ``[B, n, ...]`` that the chunk is written through.
    2. Every launch that writes or finishes those views comes before ``flush(tag)`` records ``filled[k]`` on main.
    3. ``flush``: the side stream waits on ``filled[k]``, copies each pair with ``non_blocking=True``, then records
       ``copied[k]``.  A trailing partial chunk is copied as one dense ``[B, n, ...]`` view of the same storage.
    4. ``deliver(fn)`` behind the ``flush`` of chunk ``i`` hands over chunk ``i - 1``: ``copied[j].synchronize()``, then
       ``fn(*tag, {name: pinned view})``, valid until ``fn`` returns; ``deliver(fn, keep=0)`` at the end: the last chunk.
    5. ``deliver(None)`` forgets the chunks instead: without a receiver nothing waits for the device anywhere."""

    def __init__(self, device, shapes):
        with torch.inference_mode(False):
            self.side = torch.cuda.Stream(device=device)
            self.slots = [SimpleNamespace(dev={k: torch.empty(tuple(s), device=device) for k, s in shapes.items()},
                                          host=None, filled=torch.cuda.Event(), copied=torch.cuda.Event(), used=False,
                                          open=None) for _ in range(2)]
        self.pending, self.k = [], 1       # [(slot, tag, {name: pinned view})], oldest first; the slot that is open

    def pin(self) -> "ChunkRing":
        with torch.inference_mode(False):
            for s in self.slots:
                s.host = s.host or {k: torch.empty(t.shape, pin_memory=True) for k, t in s.dev.items()}
        return self

    def open(self, n: int):
        self.k ^= 1
        s = self.slots[self.k]
        if s.used:
            torch.cuda.current_stream().wait_event(s.copied)     # the side stream has finished reading this slot
        s.open = {name: _chunk(t, n) for name, t in s.dev.items()}
        return s.open

    def flush(self, tag) -> None:
        s = self.slots[self.k]
        s.filled.record(torch.cuda.current_stream())
        host = {name: _chunk(s.host[name], d.shape[1]) for name, d in s.open.items()}
        with torch.cuda.stream(self.side):
            self.side.wait_event(s.filled)
            for name, h in host.items():
                h.copy_(s.open[name], non_blocking=True)
            s.copied.record(self.side)
        s.used = True
        self.pending.append((s, tag, host))

    def deliver(self, fn, keep: int = 1) -> None:
        while len(self.pending) > keep:
            s, tag, host = self.pending.pop(0)
            if fn is not None:
                s.copied.synchronize()
                fn(*tag, host)
