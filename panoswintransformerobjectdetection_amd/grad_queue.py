"""The end-of-pass gradient queue: parameter-gradient reductions, weight gradients and attention table gradients that a backward
pass holds back and issues as a few grouped launches when it ends (set_deferred_reductions).

Host logic over torch's autograd plus the three grouped C-ABI launches.  Every feature switch stays in ops.py, which passes its
decisions in as arguments; ops re-exports the public functions."""
import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import PswinError, call, dtype_code


def _addr(t):
    return None if t is None else t.data_ptr()


# job records: one per grouped entry point, fields named after the ctypes struct that fill() writes
class Reduction(NamedTuple):
    """dst[c] = sum_{r < rows} src.flatten()[r * ld + c], reading from `offset` bytes into src (_lib.ReduceJob)"""
    src: torch.Tensor
    offset: int
    dtype: int
    rows: int
    cols: int
    ld: int
    dst: torch.Tensor

    @property
    def ref(self):       # the tensor whose device and stream the launch runs on
        return self.src

    def fill(self, a):
        a.src, a.dst, a.dtype, a.rows, a.cols, a.ld = self.src.data_ptr() + self.offset, self.dst.data_ptr(), self.dtype, self.rows, self.cols, self.ld


class WeightGrad(NamedTuple):
    """partial[s] = dy[rows of split s]^T x, and dbias_partial[s] = the column sums of those rows of dy if given (_lib.TnJob).
    sample_scale / rows_per_sample: the sample liveness of the rows (include/pswin.h) or None / 0; the record keeps the factor vector
    referenced until the launch, like the operands."""
    dy: torch.Tensor
    x: torch.Tensor
    partial: torch.Tensor
    dbias_partial: Optional[torch.Tensor]
    M: int
    N: int
    K: int
    splits: int
    zero_lo: int
    zero_hi: int
    sample_scale: Optional[torch.Tensor] = None
    rows_per_sample: int = 0

    @property
    def ref(self):
        return self.dy

    def fill(self, a):
        a.dy, a.x, a.partial, a.dbias_partial = self.dy.data_ptr(), self.x.data_ptr(), self.partial.data_ptr(), _addr(self.dbias_partial)
        a.M, a.N, a.K, a.splits, a.partial_dtype, a.zero_lo, a.zero_hi = self.M, self.N, self.K, self.splits, dtype_code(self.partial), self.zero_lo, self.zero_hi
        a.sample_scale, a.rows_per_sample = _addr(self.sample_scale), self.rows_per_sample if self.sample_scale is not None else 0


class TableGrad(NamedTuple):
    """dalpha / dbeta of one attention module from its dScore tiles (_lib.TableGradJob).  partials_deferred (queued jobs only): the
    partial-row sums (stage 1) wait for the end of the pass as well, instead of having run where the job was queued."""
    dscore_sum: torch.Tensor
    dist_tiles_t: Optional[torch.Tensor]
    dalpha: Optional[torch.Tensor]
    dbeta: torch.Tensor
    workspace: torch.Tensor
    n_tiles: int
    n_bias_windows: int
    n_dist: int
    heads: int
    partials_deferred: bool = True

    @property
    def ref(self):
        return self.dscore_sum

    def fill(self, a):
        a.dscore_sum, a.dist_tiles_t = self.dscore_sum.data_ptr(), _addr(self.dist_tiles_t)
        a.dalpha, a.dbeta, a.workspace = _addr(self.dalpha), self.dbeta.data_ptr(), self.workspace.data_ptr()
        a.n_tiles, a.n_bias_windows, a.n_dist, a.heads = self.n_tiles, self.n_bias_windows, self.n_dist, self.heads


# the grouped launches
def _launch_grouped(name, struct, jobs, *args, key=None, booked=None):
    """One call of entry point `name` per device, over that device's jobs as an array of `struct` (in `key` order; the sort is
    stable).  booked(jobs): the timing-table keywords of _lib.call for that launch."""
    by_dev = {}
    for j in jobs:
        by_dev.setdefault(j.ref.device, []).append(j)
    for lst in by_dev.values():
        if key is not None:
            lst = sorted(lst, key=key)
        arr = (struct * len(lst))()
        for a, j in zip(arr, lst):
            j.fill(a)
        call(name, lst[0].ref, ctypes.cast(arr, ctypes.c_void_p), len(lst), *args, **(booked(lst) if booked else {}))


def _launch_reductions(jobs):
    _launch_grouped("pswin_reduce_jobs", _lib.ReduceJob, jobs)


def _launch_table_grads(jobs, stages=3):
    _launch_grouped("pswin_attn_table_grads_batch", _lib.TableGradJob, jobs, stages)


def _wgrad_traffic(jobs):
    nbytes = flops = pbytes = 0
    for j in jobs:
        nbytes += 2 * (j.M * j.K + j.M * j.N) + 4 * j.N * j.K
        flops += 2 * j.M * j.K * j.N
        pbytes += j.partial.element_size() * j.splits * j.N * j.K if j.splits > 1 else 0
    return dict(algo_bytes=nbytes, algo_flops=flops, timed_as="pswin_gemm_tn_ring", partial_bytes=pbytes)


def weight_grad(dy, x, partial, dbias_partial, splits, zero_lo=0, zero_hi=0, live=None):
    """The WeightGrad record of dy^T x; live: None or (sample_scale f32 [B] on the device, rows_per_sample)."""
    scale, rps = (None, 0) if live is None else (live[0], int(live[1]))
    return WeightGrad(dy, x, partial, dbias_partial, dy.shape[0], dy.shape[1], x.shape[1], splits, zero_lo, zero_hi, scale, rps)


def _launch_wgrads(jobs):
    """The queued weight gradients as ONE pswin_gemm_tn_ring_jobs call per device (one kernel launch per tile geometry): longest row
    ranges first, so that the tail of the launch is made of the short ones."""
    _launch_grouped("pswin_gemm_tn_ring_jobs", _lib.TnJob, jobs, key=lambda j: -(j.M // j.splits), booked=_wgrad_traffic)


# per-pass state
class _PassQueue:
    """What one backward pass has held back so far."""

    def __init__(self):
        self.reductions, self.wgrads, self.tables = [], [], []
        self.owners = set()          # data_ptr of every parameter that already has a postponed gradient in this pass

    def add_reduction(self, src, rows, cols, dst, ld=None, offset=0):
        self.reductions.append(Reduction(src, offset, dtype_code(src), rows, cols, cols if ld is None else ld, dst))

    def add_weight_gradient(self, dy, x, partial, dbias_partial, splits, zero_lo=0, zero_hi=0, live=None):
        """The operands (and the factor vector of live = (sample_scale, rows_per_sample)) stay referenced by the queue until the launch."""
        self.wgrads.append(weight_grad(dy, x, partial, dbias_partial, splits, zero_lo, zero_hi, live))

    def add_table_gradient(self, job, partial_sums):
        """job: a TableGrad; partial_sums: the Reduction between its two stages."""
        self.reductions.append(partial_sums)
        self.tables.append(job)

    def launch(self):
        jobs, tjobs, wjobs = self.reductions, self.tables, self.wgrads
        self.reductions, self.tables, self.wgrads = [], [], []
        if wjobs:
            _launch_wgrads(wjobs)                           # the reductions below sum their partial slabs
        early = [j for j in tjobs if j.partials_deferred]
        if early:
            _launch_table_grads(early, 1)                   # partial-row sums of every attention module's dScore tiles, one launch
        if jobs:
            _launch_reductions(jobs)
        if tjobs:
            _launch_table_grads(tjobs, 4)                   # per-bin sums from the partial-row sums the reductions just wrote


_enabled = False
# autograd graph task id -> _PassQueue of that backward pass.  Keyed by task because passes nest (the backward of a
# torch.utils.checkpoint segment is a pass of its own inside the outer one); each pass flushes its own jobs.
_tasks = {}
_slots = {}              # graph task id -> flat-gradient slots already handed out in that pass (grad_slot)


def _trim(d):            # leftovers of passes that raised: keep the table small (task ids grow monotonically)
    while len(d) > 8:
        del d[min(d)]


def pending():
    """The ids of the backward passes that still hold a queue (none once every pass has ended normally)."""
    return sorted(_tasks)


def _graph_task_id():
    """id of the running backward pass (-1 outside one).  A private torch entry point (present in torch 2.1 .. 2.10): without it
    nothing is postponed and no gradient slot is handed out -- every reduction launches where it is issued."""
    f = getattr(torch._C, "_current_graph_task_id", None)
    return f() if f is not None else -1


def deferred_reductions_available():
    """The two private torch entry points the end-of-pass grouping relies on (the id of the running backward pass and the
    autograd engine's end-of-pass callback) exist in this torch build."""
    eng = getattr(torch.autograd.Variable, "_execution_engine", None)
    return hasattr(torch._C, "_current_graph_task_id") and eng is not None and hasattr(eng, "queue_callback")


def set_deferred_reductions(on):
    """on=True: reductions whose result is a PARAMETER gradient (split-K partials of dW, bias-gradient partial rows,
    LayerNorm dgamma / dbeta rows) are queued while autograd runs and issued as one grouped launch when the backward pass
    ends (an autograd engine callback), instead of ~120 launches of 5-8 us each.  A postponed gradient tensor is filled
    only once backward() returns, so a reduction is postponed only when nothing can read its result earlier: the
    call site names the parameter(s) the result belongs to (``owners``), and the launch stays immediate when an owner
    already holds a ``.grad`` (autograd would accumulate into it at once), carries a tensor / post-accumulate hook
    (dp.GradReducer(pack=False) launches its all-reduce from one), or already received a postponed gradient in the same
    pass (a module applied twice: autograd adds the two as soon as the second arrives; the queue is flushed first).
    NOT covered: hooks registered on a parameter's AccumulateGrad NODE (torch DistributedDataParallel's reducer,
    ``grad_fn.register_hook`` consumers) are invisible from Python and would read unfilled gradients -- use dp.GradReducer (which
    this mode is built for) or leave deferral off under DDP.  Returns the previous setting."""
    global _enabled
    if on and not deferred_reductions_available():
        raise PswinError("set_deferred_reductions(True) needs torch._C._current_graph_task_id and the autograd engine's queue_callback "
                         f"(private entry points, present in torch 2.1 - 2.10; this is torch {torch.__version__})")
    prev, _enabled = _enabled, bool(on)
    return prev


def flush_reductions(task=None):
    """Issue the reductions queued by one backward pass (runs by itself when that pass ends); task=None: all of them."""
    keys = list(_tasks) if task is None else [task]
    for k in keys:
        q = _tasks.pop(k, None)
        if q is not None:
            q.launch()


def _has_hooks(p):
    return bool(getattr(p, "_post_accumulate_grad_hooks", None)) or bool(getattr(p, "_backward_hooks", None))


def deferring(owners=()):
    """The job queue of the running backward pass if the reduction that produces the gradients of `owners` (parameters)
    may be postponed to the end of that pass (see set_deferred_reductions; the end-of-pass callback is armed on first
    use), else None = launch now.  Without owners the destination is unknown and nothing is postponed."""
    task = _graph_task_id() if _enabled else -1
    owners = [o for o in owners if o is not None]
    if task == -1 or not owners:
        return None
    if any((not o.is_leaf) or o.grad is not None or _has_hooks(o) for o in owners):
        return None                  # a non-leaf "owner" feeds further autograd nodes right away
    q = _tasks.get(task)
    if q is None:
        q = _tasks[task] = _PassQueue()
        _trim(_tasks)
        torch.autograd.Variable._execution_engine.queue_callback(lambda: flush_reductions(task))
    keys = [o.data_ptr() for o in owners]
    if any(k in q.owners for k in keys):
        q.launch()                   # second gradient of a parameter in one pass: autograd adds it to the first one now
        return None
    q.owners.update(keys)
    return q


def flush_if_pending(owners=()):
    """A gradient of `owners` is about to be returned to autograd WITHOUT going through the queue (a weight gradient small enough
    for one launch): if an earlier use of the same parameter in this pass left a postponed (still unfilled) gradient in the queue,
    autograd would add the two at once -- issue the queue first.  (A module applied to one large and one small input.)"""
    if not _enabled:
        return
    q = _tasks.get(_graph_task_id())
    if q is not None and any(o is not None and o.data_ptr() in q.owners for o in owners):
        q.launch()


def grad_slot(param):
    """The flat-gradient-buffer view dp.GradReducer(pack=True) reserved for `param` (``param._grad_slot``) if this backward
    pass may write the parameter's gradient straight into it: the parameter holds no gradient yet (nothing to accumulate
    into), has no hooks, and the slot has not been handed out earlier in the same pass (a weight used twice gets a
    private buffer the second time and autograd adds the two).  None otherwise."""
    slot = getattr(param, "_grad_slot", None)
    if slot is None or not param.is_leaf or param.grad is not None or slot.device != param.device or _has_hooks(param):
        return None
    task = _graph_task_id()
    if task == -1:
        return None
    used = _slots.get(task)
    if used is None:
        used = _slots[task] = set()
        _trim(_slots)
    if slot.data_ptr() in used:
        return None
    used.add(slot.data_ptr())
    return slot


def sum_rows(src, rows, cols, ld=None, col_offset=0, out=None, owners=()):
    """f32 [cols]: out[c] = sum_{r < rows} src.flatten()[r * ld + col_offset + c] in a fixed order (pswin_reduce_jobs).
    owners: the parameters whose gradient the result is; inside a backward pass with set_deferred_reductions(True) the
    launch is then postponed to the end of that pass when that is safe (deferring).
    out: an existing contiguous f32 buffer of `cols` elements to write (see grad_slot); a fresh view of it is returned."""
    ld = cols if ld is None else ld
    if not src.is_contiguous():
        raise PswinError("sum_rows expects a contiguous source")
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=src.device)
    elif out.dtype != torch.float32 or out.numel() != cols or not out.is_contiguous():
        raise PswinError("sum_rows: `out` must be a contiguous float32 buffer of `cols` elements")
    q = deferring(owners)
    if q is None:
        _launch_reductions([Reduction(src, col_offset * src.element_size(), dtype_code(src), rows, cols, ld, out)])
    else:
        q.add_reduction(src, rows, cols, out, ld=ld, offset=col_offset * src.element_size())
    # the queue keeps `out` alive until the launch; hand autograd a fresh view so that AccumulateGrad can still adopt
    # the buffer as param.grad (it clones tensors that have other owners)
    return out.view(cols)


def table_gradients(gsum, dist_tiles_t, n_tiles, n_bias_windows, n_dist, heads, owners, defer_partials):
    """(dalpha or None, dbeta), f32 [169, heads]: the gradients of an attention module's two tables (owners) from the dScore tile
    sums `gsum` of its backward kernel and the transposed distance tiles (None: no great-circle table).  Three steps: partial-row
    sums of the tiles (stage 1), the sum of those rows (a reduction), per-bin sums (stage 4).
    With deferred reductions the whole table gradient waits for the end of the pass: ONE launch sums the dScore tiles of all
    attention modules (defer_partials; twelve launches of 9-15 us per step were mostly ramp; the tiles -- 16 KB per work item and
    head, ~190 MB per PanoSwin-T step at batch 8 -- stay referenced by the queue until then), the sum of its partial rows joins the
    grouped reduction and ONE binning launch follows (same kernels, same per-module decomposition either way: bitwise equal results)."""
    lib = _lib.load()
    dbeta = torch.empty(169, heads, dtype=torch.float32, device=gsum.device)
    dalpha = torch.empty_like(dbeta) if dist_tiles_t is not None else None
    ws = torch.empty(lib.pswin_attn_table_grads_workspace(heads), dtype=torch.float32, device=gsum.device)
    ld = ws.numel() // 129
    partial_sums = Reduction(ws, 0, _lib.F32, lib.pswin_attn_table_grads_partial_rows(n_tiles, heads), ld, ld, ws[128 * ld:])
    q = deferring(owners)
    job = TableGrad(gsum, dist_tiles_t, dalpha, dbeta, ws, n_tiles, n_bias_windows, n_dist, heads,
                    partials_deferred=q is not None and defer_partials)
    if not job.partials_deferred:
        _launch_table_grads([job], 1)
    if q is None:
        _launch_reductions([partial_sums])
        _launch_table_grads([job], 4)
        return dalpha, dbeta
    q.add_table_gradient(job, partial_sums)
    return (None if dalpha is None else dalpha.view(169, heads)), dbeta.view(169, heads)       # fresh views: see sum_rows
