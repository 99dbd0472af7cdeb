"""Gradient destinations and the DEFERRED per-pass launches of the backward pass: the GroupNorm gamma / beta column sums
and the Winograd weight-gradient slab sums (one table-driven launch per flush instead of ~70 / ~65 small ones), the
gradient-arena slot lookup, and the descriptor tables a HIP-graph capture of the iteration records its launches on."""
import ctypes
import functools

import torch

from .. import _lib, reducer
from .state import st
from .core import _call, _launch, _ptr, _stream


# Per-(view, channel) map sums of a gradient tensor that a kernel already had in registers: the GroupNorm backward
# knows sum_hw(dx) in closed form, and dx is exactly the dY of the conv in front of it, whose bias / embedding-bias
# gradients are those sums; a residual 1x1 conv sees the same dY tensor as the 3x3 conv it is added to.  The sums
# travel ON the gradient tensor itself (a Python attribute; autograd hands the same tensor object from one backward
# node to the next), stamped with the tensor's version: no global table, nothing keyed on addresses, and a gradient
# that autograd had to re-materialise (an accumulation) simply does not carry them.  st.ROWSUM_FUSION = False disables.


def _rowsum_put(t, rowsum, colsum):
    if st.ROWSUM_FUSION:
        t._vf_sums = (t._version, rowsum, colsum)


def _rowsum_get(t):
    h = getattr(t, "_vf_sums", None) if st.ROWSUM_FUSION else None
    if h is None or h[0] != t._version:
        return None
    return h


def _gslot(p):
    """Parameter p's slot in the data-parallel gradient arena (reducer.py), or None: the backward kernels write a
    gradient there directly so that neither autograd nor the reducer has to copy it."""
    a = reducer.ACTIVE
    return a.slot(p) if (a is not None and p is not None) else None


def _gout(p, *shape, like):
    t = _gslot(p)
    return t if t is not None else torch.empty(*shape, device=like.device, dtype=torch.float32)


# GroupNorm weight / bias gradients = column sums over the views of the per-(view, channel) partials the backward kernel
# emits: ~70 launches of 5 us per backward pass.  They are deferred: every GroupNorm backward only registers its
# (partials, destination) pair, and ONE multi-tensor launch fills all destinations -- at the end of the backward pass (an
# autograd engine callback) in single-process training, or, with the data-parallel gradient arena, right before a
# segment's all-reduce is issued (reducer.GradArena calls flush_deferred(): ~6 launches per pass instead of 73).
# Deferral hands autograd a destination that is FILLED LATER, so it is only taken when nothing can read the gradient
# before the flush:
#   * both parameters' .grad is None (AccumulateGrad then adopts the tensor without reading it; zero_grad(set_to_none=
#     True), what Trainer.step does);
#   * no tensor hook / post-accumulate-grad hook sits on the parameters (the arena's own hooks are the exception -- the
#     post-accumulate hook of the eager step and the tensor hook on a leaf alias of the captured step: both flush before
#     they let a segment go);
#   * the parameter is not marked `_vf_no_defer`: torch's DistributedDataParallel copies a gradient into its bucket from
#     a hook on the AccumulateGrad NODE (invisible from the tensor) while the backward pass is still running, so Trainer
#     marks the parameters of a model it wraps in DDP (VF_REDUCER=ddp); st.COLSUM_DEFER = False switches deferral off
#     for the whole process (nothing in the package sets it).
# A backward pass that raises never runs its engine callbacks, and a re-entrant backward pass (torch.utils.checkpoint)
# starts a new graph task while the outer one still has entries pending: entries of another task are recognised by their
# graph-task id and FLUSHED by the next pass (filling a destination nobody will read is harmless; dropping one autograd
# still hands out is not).  A capture that aborts drops them explicitly (drop_deferred).
# Round 5: the slab sums behind the Winograd weight-gradient kernels (65 launches of ~7 us per iteration) are deferred the
# same way -- every layer runs only its main kernel into a workspace of its own (vf_wino_wgrad_main) and registers a
# descriptor row; ONE vf_wino44_reduce_multi launch per flush fills dW (and the bias gradients that ride along).  Same
# conditions, same flush points, same graph-task bookkeeping as the GroupNorm sums.  VF_WRED_DEFER=0: tuning aid.
# The deferred layers' slab workspaces (~18 MiB each, ~1.15 GiB per backward pass at S = 96) are slices of ONE
# per-device arena that every pass -- eager or replayed, whatever its geometry -- fills from offset 0: passes are
# ordered on the stream and a pass's slabs are dead once its flush has run.  (Round 5 gave every layer a fresh tensor:
# inside a captured iteration that pinned 1.15 GiB per graph -- a ragged run holds up to B (N - 1) + 1 graphs.)
# The arena grows outside captures only (a new, larger tensor; slices already handed out keep the old one alive until
# their flush, and a graph keeps the arena it was captured with); a captured layer that does not fit runs the
# non-deferred launch instead.


class _Arena:
    """The slab arena of one device: the tensor (None until the first deferred layer) and the floats handed out in the
    running backward pass."""

    def __init__(self):
        self.buf, self.used = None, 0


def _wred_ws(device, need):
    """`need` floats of the slab arena for one layer of the running backward pass, or None (inside a capture, arena
    too small: the caller launches the non-deferred kernel pair)."""
    a = st._WRED_ARENA.setdefault(device, _Arena())
    n = (int(need) + 63) // 64 * 64
    cap = 0 if a.buf is None else a.buf.numel()
    if a.used + n > cap:
        if torch.cuda.is_current_stream_capturing():
            return None
        # (the slices of the old arena stay valid: the pending entries reference them)
        a.buf = torch.empty(max(2 * cap, a.used + n, 1 << 24), device=device, dtype=torch.float32)
        a.used = 0
    ws = a.buf[a.used:a.used + n]
    a.used += n
    return ws


def wred_arena_bytes(device=None):
    """Bytes of the slab arena(s) currently allocated (tools/long_run.py reports it)."""
    return sum(4 * a.buf.numel() for d, a in st._WRED_ARENA.items() if a.buf is not None and (device is None or d == device))


_CS_RING = 16           # staging buffers in rotation (the gradient arena flushes once per segment: ~6 tables per pass)


# A captured training step (train.Trainer) launches its table-driven kernels on device tables whose CONTENTS are only
# needed when the graph is replayed: they are uploaded after the capture has ended, with ordinary copies -- no host-to-
# device copy node (and no pinned staging buffer to keep stable) inside the graph.  Such a table must NOT come from the
# capturing graph's memory pool: the pool hands a block that an earlier tensor of the same capture has released to a
# later one, so on every replay the earlier kernels would scribble over a table uploaded once.  begin_capture()
# therefore allocates the table BEFORE the capture starts.


class _CaptureTable:
    def __init__(self, table):
        self.table = table      # device rows, allocated before the capture
        self.used = 0           # rows the flushes of the capture have taken so far
        self.rows = []          # their contents, uploaded by end_capture
        self.keep = []          # the flushed pending lists: their tensors live as long as the graph's owner keeps this


class _Slot:
    """One staging table of a family's ring: the rows of one flush, uploaded once and launched on for as long as the
    caching allocator hands the same addresses back."""

    def __init__(self):
        self.pinned = self.table = self.key = None
        self.event = torch.cuda.Event()     # recorded behind the upload
        self.rows = self.workgroups = 0


class _Deferred:
    """One family of deferred launches: the entries registered by the running backward pass, and the ONE table-driven
    launch per flush that serves them all.
        width      int64 words per table row
        launch     launch(table pointer, rows, workgroups, stream): the family's C-ABI entry point
        rows_of    pure function: pending list -> (rows, total workgroups)
        key_of     pending list -> what an uploaded table is recognised by (the addresses and sizes in its rows)
        full       the error of a capture whose table is missing or too small"""

    def __init__(self, width, launch, rows_of, key_of, full):
        self.width, self.launch, self.rows_of, self.key_of, self.full = width, launch, rows_of, key_of, full
        self.pending = []       # entries of the running backward pass (of graph task st._PENDING_TASK)
        self.device = None      # ... and the device their tensors live on
        self.capture = None     # _CaptureTable while a Trainer is capturing
        self.rings = {}         # device -> [_Slot], at most _CS_RING, the one the next miss overwrites first
        self.keep = None        # the entries of the last eager flush: what its launch still reads

    def add(self, device, entry):
        self.pending.append(entry)
        self.device = device

    def begin_capture(self, device, max_rows):
        self.capture = _CaptureTable(torch.empty(max(1, max_rows), self.width, dtype=torch.int64, device=device))

    def end_capture(self):
        ct, self.capture = self.capture, None
        if ct is not None and ct.used:
            ct.table[:ct.used].copy_(torch.tensor(ct.rows, dtype=torch.int64))
        return ct

    def flush(self):
        pend, self.pending = self.pending, []
        if not pend:
            return
        if torch.cuda.is_current_stream_capturing():
            # (several flushes per capture with the gradient arena: each takes the next rows of the pre-allocated table)
            ct = self.capture
            rows, total = self.rows_of(pend)
            if ct is None or ct.used + len(rows) > ct.table.shape[0]:
                raise _lib.VFHipError(self.full)
            self.launch(ctypes.c_void_p(ct.table.data_ptr() + 8 * self.width * ct.used), len(rows), total, _stream())
            ct.used += len(rows)
            ct.rows += rows
            ct.keep.append(pend)
            return
        key = self.key_of(pend)
        ring = self.rings.setdefault(self.device, [])
        # the caching allocator cycles through a few address sets: reuse an uploaded table
        slot = next((s for s in ring if s.key == key), None)
        if slot is None:
            rows, total = self.rows_of(pend)
            if len(ring) < _CS_RING:
                slot = _Slot()
            else:
                slot = ring.pop(0)
                slot.event.synchronize()      # that buffer's last upload is at least _CS_RING flushes old: no wait
            ring.append(slot)
            if slot.pinned is None or slot.pinned.shape[0] < len(rows):
                n = max(128, len(rows))
                slot.pinned = torch.empty(n, self.width, dtype=torch.int64).pin_memory()
                slot.table = torch.empty(n, self.width, dtype=torch.int64, device=self.device)
            slot.pinned[:len(rows)].copy_(torch.tensor(rows, dtype=torch.int64))
            slot.table[:len(rows)].copy_(slot.pinned[:len(rows)], non_blocking=True)
            slot.event.record()
            slot.key, slot.rows, slot.workgroups = key, len(rows), total
        self.launch(ctypes.c_void_p(slot.table.data_ptr()), slot.rows, slot.workgroups, _stream())
        self.keep = pend                # partials / workspaces / destinations stay referenced until the next flush


def _wred_rows(pend):
    """Slab sums, entries (row the main kernel's launcher wrote, its workgroups, (ws, dw, db, db2) to keep alive)."""
    rows, first = [], 0
    for row, nblk, _ in pend:
        r = list(row)
        r[8] = (r[8] & ~0xFFFFFFFF) | first          # `first` = the int32 at byte 64 of the row
        rows.append(r)
        first += nblk
    return rows, first


def _colsum_rows(pend):
    """Column sums, entries (parts, dgb, batch, S, C): `batch` sums of C columns over S rows each, 64 columns a workgroup."""
    rows, first = [], 0
    for parts, dgb, batch, S, C in pend:
        rows.append([parts.data_ptr(), dgb.data_ptr(), S, C, batch, first])
        first += ((C + 63) // 64) * batch
    return rows, first


st.slab_sums = _Deferred(
    9, functools.partial(_launch, "conv_wgrad", 0.0, "vf_wino44_reduce_multi"), _wred_rows,
    lambda pend: tuple(v for row, _, _ in pend for v in row),
    "deferred weight-gradient slab sums inside a stream capture need ops.begin_capture() "
    "with max_conv_rows >= the number of 3x3 layers (one backward pass per capture)")
st.col_sums = _Deferred(
    6, functools.partial(_call, "vf_colsum_multi"), _colsum_rows,
    lambda pend: tuple(v for parts, dgb, _, S, C in pend for v in (parts.data_ptr(), dgb.data_ptr(), S, C)),
    "deferred GroupNorm parameter sums inside a stream capture need ops.begin_capture() "
    "with room for every GroupNorm layer (one backward pass per capture)")


def begin_capture(device, max_rows, max_conv_rows=0):
    st.col_sums.begin_capture(device, max_rows)
    if max_conv_rows:
        st.slab_sums.begin_capture(device, max_conv_rows)
    else:
        st.slab_sums.capture = None


def end_capture():
    """Upload the tables of the capture that just ended; returns what the graph's owner must keep referenced for as
    long as it replays the graph."""
    drop_deferred()                 # (only a capture that failed half-way leaves any)
    return st.col_sums.end_capture(), st.slab_sums.end_capture()


def _flush():
    st.slab_sums.flush()
    for a in st._WRED_ARENA.values():       # the next pass fills the arena from its start again (stream order)
        a.used = 0
    st._PENDING_TASK = None
    st.col_sums.flush()


def _defer_ok(params):
    a = reducer.ACTIVE
    flushes = a is not None and getattr(a, "flushes_colsums", False)
    for p in params:
        if p is None or p.grad is not None or getattr(p, "_vf_no_defer", False):
            return False
        if getattr(p, "_backward_hooks", None) and not (flushes and id(p) in a._alias):
            return False        # a foreign tensor hook would read the gradient before the flush; the arena's own hook
                                # on a leaf alias (captured iteration) flushes before it lets the segment go
        if a is None and getattr(p, "_post_accumulate_grad_hooks", None):
            return False
    return a is None or flushes


def _colsum(parts, dgb, batch, S, C, params):
    """dgb[b][c] = sum_s parts[b][s][c], now or (see above) deferred to the flush of the running backward pass."""
    # (entries of another graph task: a backward pass that failed (its callback never ran) -- or the OUTER pass of a
    # re-entrant backward (torch.utils.checkpoint, autograd.grad inside a backward), whose destinations autograd will still
    # hand out.  Outside a capture filling them now is always right (the entries keep their tensors alive); inside a
    # capture the abort path has already dropped them (drop_deferred).  _defer_begin does that.)
    if _defer_begin(params, st.col_sums):
        st.col_sums.add(parts.device, (parts, dgb, batch, S, C))
        return
    _call("vf_colsum", _ptr(parts), _ptr(dgb), batch, S, C, _stream())


def _defer_begin(params, family):
    """Common entry of the two deferrals: True when a destination may be filled at the flush of the running backward
    pass; makes sure that flush is queued and that entries of another graph task are dealt with first."""
    task = torch._C._current_graph_task_id()
    if not (st.COLSUM_DEFER and task != -1 and _defer_ok(params)
            and (family.capture is not None or not torch.cuda.is_current_stream_capturing())):
        return False
    if (st.col_sums.pending or st.slab_sums.pending) and st._PENDING_TASK != task:
        if torch.cuda.is_current_stream_capturing():
            st.col_sums.pending.clear()
            st.slab_sums.pending.clear()
        else:
            _flush()
    if not st.col_sums.pending and not st.slab_sums.pending:
        st._PENDING_TASK = task
        torch.autograd.Variable._execution_engine.queue_callback(_flush)
    return True


def flush_deferred():
    """Fill the destinations registered so far, GroupNorm sums and weight gradients alike (the gradient arena calls
    this before a segment's all-reduce)."""
    if st.col_sums.pending or st.slab_sums.pending:
        _flush()


def drop_deferred():
    """Forget deferred sums of a backward pass that did not complete (capture failure paths)."""
    st.col_sums.pending.clear()
    st.slab_sums.pending.clear()
    st._PENDING_TASK = None
    for a in st._WRED_ARENA.values():
        a.used = 0
