"""Steps replayed from a captured hipGraph: the ONE copy of the capture protocol, of the eager-first rule and of what a
captured training step does around its body ("Captured steps").  The four training steps of
engine.py, lineval.HeadStep and cddls.CDDLSSampler all capture through here."""
import torch
import torch.distributed as dist

from . import ops
from .hostio import THROTTLE, upload_into


def quiesce_before_capture(*modules):
    """Called right before a stream capture; returns the ``capture_error_mode`` to capture with.

    With a process group, every EAGER collective issued so far is still listed in ProcessGroupNCCL's watchdog thread until
    that thread has seen it complete (it polls every 100 ms).  The capture pulls RCCL's own stream into capture mode, and
    under the default 'global' capture mode ``hipEventQuery`` from ANY thread is then refused ("operation not permitted on
    an event last recorded in a capturing stream") -- the watchdog rethrows and the whole job aborts.  Seen once in nine
    runs of tests/dist_graph_worker.py, on a cold box where the watchdog had not drained yet.  Deterministic part: with a
    process group the capture runs in 'thread_local' mode, in which only THIS thread's calls are policed, so the watchdog
    thread may keep polling whatever it still holds.  Belt and braces: the device is drained first and the watchdog gets a
    moment to retire the eager works (there is no API to wait for that)."""
    for m in modules:                       # no autograd graph of an eager step may stay referenced across the capture
        if hasattr(m, 'drop_pack_cache'):
            m.drop_pack_cache()
    torch.cuda.synchronize()
    if dist.is_available() and dist.is_initialized():
        import time
        time.sleep(1.0)          # (the full second stays until thread_local mode is proven on W > 1 hardware)
        torch.cuda.synchronize()
        return 'thread_local'
    return 'global'


def capture(body, modules, scratch):
    """Record ``body()`` into a new hipGraph -> (graph, what the body returned).  ``modules``: see quiesce_before_capture;
    ``scratch``: the dict that holds this graph's own conv workspaces (ops.private_workspace) -- the caller keeps it alive
    with the graph.  Capture records launches, it does not run them: the body's inputs stay untouched and what it
    allocated is filled by the first replay."""
    mode = quiesce_before_capture(*modules)
    if ops.SEQUENCE is not None:
        ops.SEQUENCE.append('capture')          # (bench.py --shape-table: the launch order of the captured step follows)
    graph = torch.cuda.CUDAGraph()
    with ops.private_workspace(scratch), torch.cuda.graph(graph, capture_error_mode=mode):
        result = body()
    torch.cuda.synchronize()
    return graph, result


class EagerFirst(object):
    """The eager-first rule: a step is captured at its second use in THIS process at the earliest, and, where an optimizer
    is involved, only once that optimizer holds state.  The state alone is not enough: after ``--resume`` it is non-empty
    at once, but the first step of a fresh process still does first-use host work that must not land inside a stream
    capture (blocking host -> device copies of cached constants, first-time workspace allocations, kernel module loads)."""

    def __init__(self):
        self.eager = 0                      # eager uses counted in this process

    def may_capture(self, optimizer=None, counts=True):
        """True: capture (or replay) now.  False: run this use eagerly; it is counted unless ``counts`` is False -- a use
        that differs from the step to be captured (cDDLS with explicit noise) neither counts nor captures."""
        if counts and self.eager >= 1 and (optimizer is None or len(optimizer.state) > 0):
            return True
        self.eager += 1 if counts else 0
        return False


def _detached(x):
    if isinstance(x, dict):
        return {k: _detached(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(_detached(v) for v in x)
    return x.detach()


class CapturedStep(object):
    """A step on static device buffers, captured once and replayed by every call.  Subclasses supply ``_refresh()`` (new
    contents for the static inputs, drawn on the host in the eager path's RNG order) and ``_body()`` (the launches), and
    call ``_capture()`` at the end of their constructor."""

    def _capture(self, quiesce=(), repack=()):
        """``repack``: modules whose packed weights the body has to rebuild itself, because they move between two replays
        (``invalidate_cache()`` before the capture, so that the pack launches are RECORDED, and after it, because the
        buffers a capture allocated hold nothing until the first replay)."""
        for m in repack:
            m.invalidate_cache()
        self._scratch = {}
        self.graph, self.result = capture(self._body, quiesce, self._scratch)
        for m in repack:
            m.invalidate_cache()

    def __call__(self):
        THROTTLE.begin()
        self._refresh()
        self.graph.replay()
        THROTTLE.end()
        return self.result


class CapturedTrainStep(CapturedStep):
    """A captured optimizer step: loss -> backward -> [gradient all-reduce] -> fused Adam whose three step-dependent
    scalars (and the 1/W of the data-parallel mean) are read from device memory.  ``data_parallel``: engine.dist_on() at
    construction.  Subclasses supply ``_refresh_inputs()`` and end ``_body()`` with ``return self._finish(loss, result)``."""

    def __init__(self, opt, reducer, data_parallel, device):
        self.opt, self.reducer, self.dist = opt, reducer, data_parallel
        self.hyper = torch.ones(3, device=device)

    def _refresh(self):
        self._refresh_inputs()
        self._refresh_hyper()

    def _refresh_hyper(self):
        """Once per replay, no more: hyper_values() advances the optimizer's step count."""
        world = dist.get_world_size() if self.dist else 1
        upload_into(torch.tensor([self.opt.hyper_values(1.0 / world)], dtype=torch.float32), self.hyper.view(1, 3))

    def _finish(self, loss, result):
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        if self.reducer is not None:
            self.reducer()                      # (an overlapped reducer has exchanged inside the backward already)
        self.opt.step_captured(self.hyper)
        # detached: the step's autograd graph must not outlive the capture (its AccumulateGrad nodes are tied to the
        # capture stream; an eager backward later on would have to synchronise with it)
        return _detached(result)
