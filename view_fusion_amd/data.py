"""A device-resident view store: a dataset split kept on the GPU as uint8, and seeded batch assembly in one HIP launch.

The reference feeds the model from a single-worker webdataset (data/nmr_dataset.py, experiment.py:158-216): per object it
decodes 24 PNGs, shuffles the views with np.random in a worker process, builds float32 arrays, collates and copies them to
the device.  None of that has to happen per step.  An NMR-style split as uint8 is 24 x 3 x 64 x 64 B = 288 KiB per
object (about 9 GB for 30 k objects); `ViewStore` holds it as one planar (N, 24, 3, H, W) uint8 tensor, and
`store.batch(seed, ids)` turns (seed, sample ids) into exactly the batch process_sample + collate + .to(device) produce
-- csrc/batch.hip, one launch, no host sync, no allocation beyond the outputs.  Every draw (the view shuffle, the 10 %
"target among the conditioning views" re-shuffle, view_count, the object) comes from the counter-based generator of
csrc/rng.h (kind 4), so a sample is a function of (seed, sample id) alone, whatever its batch, order or rank.

Array layout the user's one-off conversion must produce (reading tars and decoding PNGs is NOT part of this package):
uint8, shape (N, 24, H, W, 3) -- object, view 0000.png ... 0023.png in that order, rows, columns, RGB -- saved with
np.save; `ViewStore.from_npy(path)` memory-maps it, uploads it in chunks and transposes it once on the device.  A planar
(N, 24, 3, H, W) array is taken with layout="planar".  H * W must be a multiple of 4.

Not built: an epoch-permutation sampler (objects are drawn with replacement, as the reference's resampled=True, or
named by the caller), and fusing the assembly into stack_views."""
import ctypes

import numpy as np
import torch

from . import _lib

VIEWS = 24


def _host_ids(ids):
    t = torch.as_tensor(ids).reshape(-1)
    if t.is_cuda:
        raise ValueError("ViewStore.batch needs the sample ids on the host (list / CPU tensor): view_count is computed "
                         "from them there, and reading a device tensor back would be a sync per batch")
    return t.to(torch.int64).contiguous()


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def host_plan(seed, ids, mode="train", view_range=(1, 6), N=1, objects=None):
    """The plan of samples `ids` under `seed` on the CPU (the library's host mirror of the kernel's plan; no GPU): a dict
    of CPU tensors src (B, 24) [cond[k] = views[src[k + 1]]], target (B,), q01 (B, 2), second (B,), view_count (B,) int64
    in view_range, object (B,) int64 (objects[b] when given).  Raises ValueError for an object outside [0, N)."""
    if seed is None:
        raise ValueError("the view store draws from the seeded generator only: seed=None is not a seed")
    if mode not in ("train", "test"):
        raise ValueError(f"mode must be 'train' or 'test', got {mode!r}")
    ids = _host_ids(ids)
    B = ids.numel()
    lo, hi = (int(v) for v in view_range)
    if not 1 <= lo <= hi <= VIEWS - 1:
        raise ValueError(f"view_range {view_range!r} must satisfy 1 <= lo <= hi <= {VIEWS - 1}")
    if N < 1 or N >= 2 ** 32:
        raise ValueError(f"a store of {N} objects is outside [1, 2^32)")
    if objects is not None:
        objects = torch.as_tensor(objects).reshape(-1).to(torch.int64).contiguous()
        if objects.is_cuda:
            raise ValueError("objects must be on the host (list / CPU tensor): they are range-checked there")
        if objects.numel() != B:
            raise ValueError(f"one object per sample: {objects.numel()} objects for {B} ids")
        if B and (int(objects.min()) < 0 or int(objects.max()) >= N):
            raise ValueError(f"objects out of range for a store of {N} objects")
    out = dict(src=torch.empty(B, VIEWS, dtype=torch.int32), target=torch.empty(B, dtype=torch.int32),
               q01=torch.empty(B, 2, dtype=torch.int32), second=torch.empty(B, dtype=torch.int32),
               view_count=torch.empty(B, dtype=torch.int64), object=torch.empty(B, dtype=torch.int64))
    _lib.call("vf_batch_host_plan", int(seed) & 0xFFFFFFFFFFFFFFFF, _vp(ids), B, int(mode == "train"), lo, hi, int(N),
              _vp(objects), _vp(out["src"]), _vp(out["target"]), _vp(out["q01"]), _vp(out["second"]),
              _vp(out["view_count"]), _vp(out["object"]))
    return out




class ViewStore:
    """A dataset split on the device: `views` (N, 24, 3, H, W) uint8, planar, contiguous."""

    def __init__(self, views_u8):
        if not torch.is_tensor(views_u8) or views_u8.dtype != torch.uint8:
            raise ValueError(f"the store holds uint8 views, got {getattr(views_u8, 'dtype', type(views_u8))}")
        if views_u8.dim() != 5 or views_u8.shape[1] != VIEWS or views_u8.shape[2] != 3:
            raise ValueError(f"the store is planar (N, {VIEWS}, 3, H, W); got {tuple(views_u8.shape)}")
        if views_u8.shape[0] < 1:
            raise ValueError("the store holds no object")
        if (views_u8.shape[3] * views_u8.shape[4]) % 4:
            raise ValueError(f"H * W must be a multiple of 4, got {views_u8.shape[3]} x {views_u8.shape[4]}")
        self.views = views_u8.contiguous()
        self.N, _, _, self.H, self.W = self.views.shape
        self._idx = {}              # (what, B) -> device int64 (B,): ids / objects of a batch, rewritten in place

    def __len__(self):
        return self.N

    @property
    def device(self):
        return self.views.device

    @classmethod
    def from_hwc(cls, array, device="cuda", chunk=256):
        """`array`: (N, 24, H, W, 3) uint8 as decoded (numpy array or memmap).  Uploaded `chunk` objects at a time and
        transposed on the device into the planar store: the host never holds a second copy."""
        if getattr(array, "dtype", None) != np.uint8:
            raise ValueError(f"the store holds uint8 views, got {getattr(array, 'dtype', type(array))}")
        if array.ndim != 5 or array.shape[1] != VIEWS or array.shape[4] != 3:
            raise ValueError(f"from_hwc takes (N, {VIEWS}, H, W, 3); got {tuple(array.shape)}")
        N, _, H, W, _ = array.shape
        if N < 1:
            raise ValueError("the store holds no object")
        if (H * W) % 4:
            raise ValueError(f"H * W must be a multiple of 4, got {H} x {W}")
        views = torch.empty(N, VIEWS, 3, H, W, dtype=torch.uint8, device=device)
        for i in range(0, N, chunk):
            part = torch.from_numpy(np.array(array[i:i + chunk])).to(device)
            views[i:i + chunk] = part.permute(0, 1, 4, 2, 3)
        return cls(views)

    @classmethod
    def from_npy(cls, path, device="cuda", layout="hwc", chunk=256):
        """A .npy file written by the user's one-off conversion, memory-mapped: layout "hwc" (N, 24, H, W, 3), as decoded,
        or "planar" (N, 24, 3, H, W)."""
        array = np.load(path, mmap_mode="r")
        if layout == "hwc":
            return cls.from_hwc(array, device=device, chunk=chunk)
        if layout != "planar":
            raise ValueError(f"layout must be 'hwc' or 'planar', got {layout!r}")
        if array.dtype != np.uint8:
            raise ValueError(f"the store holds uint8 views, got {array.dtype}")
        if array.ndim != 5 or array.shape[1] != VIEWS or array.shape[2] != 3:
            raise ValueError(f"the store is planar (N, {VIEWS}, 3, H, W); got {tuple(array.shape)}")
        views = torch.empty(array.shape, dtype=torch.uint8, device=device)
        for i in range(0, array.shape[0], chunk):
            views[i:i + chunk] = torch.from_numpy(np.array(array[i:i + chunk])).to(device)
        return cls(views)

    def _index(self, what, t):
        """A host int64 vector on the device: one buffer per (what, length), refilled by a pinned non-blocking copy --
        stream-ordered, so the store serves one stream at a time; no allocation after the first batch of a size."""
        buf = self._idx.get((what, t.numel()))
        if buf is None:
            buf = self._idx[(what, t.numel())] = torch.empty(t.numel(), dtype=torch.int64, device=self.device)
        buf.copy_(t.pin_memory(), non_blocking=True)
        return buf

    # -- batches ----------------------------------------------------------------------------------------------------
    def _out(self, out, key, shape):
        t = None if out is None else out.get(key)
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32 or not t.is_contiguous() or \
                t.device != self.device or t.data_ptr() % 16:
            raise ValueError(f"out[{key!r}] must be a contiguous, 16-byte aligned float32 tensor of shape {tuple(shape)} "
                             "on the store's device")
        return t

    def batch(self, seed, ids, mode="train", max_views=6, relative=False, objects=None, view_count=None,
              view_range=None, out=None, return_plan=False, ids_device=None):
        """The batch of samples `ids` (list / CPU tensor, one id per sample, as ops.sample_ids takes them) under `seed`:
        {"y_0": (B,3,H,W), "y_cond": (B,23,3|6,H,W), "angle": (B,1)} on the device and "view_count": (B,) int64 on the
        CPU -- exactly the keys Trainer.step and model.forward take, nothing else.  One HIP launch; the host part is the
        library's host mirror of the plan (view_count without a sync) and two small pinned copies.
        mode "train" takes the reference's 10 % second shuffle, "test" never does.  relative: y_cond is the reference's
        relative_cond (6 channels) and angle its relative_angle.  objects (list / CPU tensor): the object of every
        sample; default: drawn from the store with replacement.  view_count: given instead of drawn.  view_range =
        (lo, hi): drawn from [lo, hi] instead of [1, max_views] ((max_views + 1, 23) is the extrapolation call shape).
        out: a dict with preallocated "y_0" / "y_cond" / "angle" to write into.  return_plan=True: -> (batch, plan), plan
        as host_plan() returns it.  ids_device: the same ids as a device int64 tensor, when the caller already has them
        there (saves the copy)."""
        plan = host_plan(seed, ids, mode, view_range or (1, int(max_views)), self.N, objects)
        self._need_gpu()
        ids_h = _host_ids(ids)
        B = ids_h.numel()
        if view_count is not None:
            vc = torch.as_tensor(view_count).reshape(-1).to(torch.int64).cpu()
            if vc.numel() != B:
                raise ValueError(f"one view_count per sample: {vc.numel()} for {B} ids")
        else:
            vc = plan["view_count"]
        C = 6 if relative else 3
        y_0 = self._out(out, "y_0", (B, 3, self.H, self.W))
        y_cond = self._out(out, "y_cond", (B, VIEWS - 1, C, self.H, self.W))
        angle = self._out(out, "angle", (B, 1))
        ids_d = self._index("ids", ids_h) if ids_device is None else ids_device
        obj_d = None if objects is None else self._index("objects", plan["object"])
        self._assemble(seed, ids_d, obj_d, B, mode == "train", relative, False, y_0, y_cond, angle)
        batch = dict(y_0=y_0, y_cond=y_cond, angle=angle, view_count=vc)
        return (batch, plan) if return_plan else batch

    def _need_gpu(self):
        if not self.views.is_cuda:
            raise _lib.VFHipError("batches are assembled by a HIP kernel from a store on the GPU (no CPU fallback): "
                                  "build the store from a device tensor, or with from_hwc / from_npy")

    def _assemble(self, seed, ids_d, obj_d, B, train, relative, all_, y_0, y_cond, angle):
        from .ops.core import _call, _stream
        _call("vf_batch_assemble", _vp(self.views), self.N, self.H, self.W, int(seed or 0) & 0xFFFFFFFFFFFFFFFF,
              _vp(ids_d), _vp(obj_d), B, int(train), int(relative), int(all_), _vp(y_0), _vp(y_cond), _vp(angle), None,
              _stream())

    def all_views(self, objects, out=None):
        """(n, 24, 3, H, W) float32: every view of `objects` (int / list / CPU tensor) in file order -- the same kernel
        with the identity plan.  all_views(i)[0] is what drivers.orbit_frames takes."""
        objects = torch.as_tensor(objects).reshape(-1).to(torch.int64)
        if objects.is_cuda:
            raise ValueError("objects must be on the host (list / CPU tensor): they are range-checked there")
        n = objects.numel()
        if n and (int(objects.min()) < 0 or int(objects.max()) >= self.N):
            raise ValueError(f"objects out of range for a store of {self.N} objects")
        self._need_gpu()
        views = self._out(None if out is None else dict(v=out), "v", (n, VIEWS, 3, self.H, self.W))
        self._assemble(0, None, self._index("objects", objects.contiguous()), n, False, False, True, None, views, None)
        return views

    def eval_batches(self, B, seed, max_views=6, rank=0, world=1, relative=False):
        """The batches drivers.evaluate(model, batches, seed=...) consumes: mode "test", objects rank, rank + world, ...
        in order, sample id = object index -- an object's views, view_count and (through "ids") sampler noise do not depend
        on B or on the sharding.  The last batch may be short."""
        if seed is None:
            raise ValueError("the view store draws from the seeded generator only: seed=None is not a seed")
        mine = list(range(rank, self.N, world))
        for i in range(0, len(mine), B):
            ids = torch.tensor(mine[i:i + B], dtype=torch.int64)
            b = self.batch(seed, ids, mode="test", max_views=max_views, relative=relative, objects=ids)
            yield dict(target=b["y_0"], cond=b["y_cond"], angle=b["angle"], view_count=b["view_count"], ids=ids)
