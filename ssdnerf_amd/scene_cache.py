"""Scene cache and its wire format.

A cached scene is the dict the reference passes between its training loop, its RAM / file cache and ``torch.save``
(reference: lib/models/autodecoders/multiscene_nerf.py:17-28 ``out_dict_to``, :74-183 ``load_cache`` / ``save_cache``;
casting helpers lib/core/utils/misc.py:43-128):

    {scene_id, scene_name,
     param:     {code_ (pre-activation, fp32 or fp16), density_grid (Morton, fp16), density_bitfield (uint8)},
     optimizer: state_dict() of the per-scene code optimizer (fp32, or bf16 in the 16-bit cache; 'step' keeps its dtype)}

``cache_16bit`` stores the code in fp16 and the optimizer moments in bf16, clamping to the target type's finite range first;
``density_grid`` / ``density_bitfield`` / ``step`` are never cast.  Test-time files written by ``BaseNeRF.save_scene`` carry the
ACTIVATED ``code`` instead of ``code_``; ``load_cache`` inverts the activation for those, ``load_scene`` uses them as they are.

``DeviceSceneCache`` holds the same state in device arrays instead of a dict of CPU tensors (``MultiSceneNeRF(cache_store='device')``): a batch
leaves and re-enters it by one HIP launch each way (csrc/scene_cache.hip), under the same casting rules, and its entries are exported in the
format above on request."""
from __future__ import annotations

import atexit
import ctypes
import os
import queue
import threading
from collections import abc as container_abcs
from collections import defaultdict
from itertools import chain
from typing import Dict, List, Optional

import torch

_UNCAST_KEYS = ("density_grid", "density_bitfield", "step")


def _clamp_to(val: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return val.clamp(min=torch.finfo(dtype).min, max=torch.finfo(dtype).max)


def optimizer_state_to(state_dict: Dict, device=None, dtype: torch.dtype = torch.float32) -> Dict:
    """Copy of an optimizer ``state_dict()`` on ``device`` with every tensor but ``step`` cast to ``dtype`` (clamped to its finite
    range when the dtype changes); ``param_groups`` is shared, not copied (misc.py:43-59)."""
    assert dtype.is_floating_point
    out = dict(state=dict(), param_groups=state_dict["param_groups"])
    for pid, st in state_dict["state"].items():
        o = dict()
        for key, val in st.items():
            if isinstance(val, torch.Tensor):
                if key != "step" and val.dtype != dtype:
                    val = _clamp_to(val, dtype)
                o[key] = val.to(device=device, dtype=None if key == "step" else dtype)
            else:
                o[key] = val
        out["state"][pid] = o
    return out


def load_tensor_to_dict(d: Dict, key: str, value, device=None, dtype: torch.dtype = torch.float32) -> None:
    """Store ``value`` under ``d[key]``: in place (``copy_``, keeping the existing tensor's dtype/device) when the key exists, else as a
    new tensor cast like ``optimizer_state_to`` does; grids, bitfields and step counters keep their dtype (misc.py:63-75)."""
    assert dtype.is_floating_point
    if isinstance(value, torch.Tensor):
        if key not in _UNCAST_KEYS and value.dtype != dtype:
            value = _clamp_to(value, dtype)
        if key in d:
            d[key].copy_(value)
        else:
            d[key] = value.to(device=device, dtype=None if key in _UNCAST_KEYS else dtype)
    else:
        d[key] = value


def optimizer_state_copy(d_src: Dict, d_dst: Dict, device=None, dtype: torch.dtype = torch.float32) -> None:
    """Refresh a cached optimizer state in place from a live ``state_dict()`` (misc.py:78-85)."""
    d_dst["param_groups"] = d_src["param_groups"]
    for pid, st in d_src["state"].items():
        if pid not in d_dst["state"]:
            d_dst["state"][pid] = dict()
        for key, val in st.items():
            load_tensor_to_dict(d_dst["state"][pid], key, val, device=device, dtype=dtype)


def optimizer_set_state(optimizer: torch.optim.Optimizer, state_dict: Dict) -> None:
    """``Optimizer.load_state_dict`` for the STATE only - the live ``param_groups`` (learning rate ...) stay as built from the current
    config (misc.py:88-128).  Moments are cast to the parameter's dtype and device, ``step`` is left alone."""
    groups, saved_groups = optimizer.param_groups, state_dict["param_groups"]
    if len(groups) != len(saved_groups):
        raise ValueError("loaded state dict has a different number of parameter groups")
    if any(len(g["params"]) != len(s["params"]) for g, s in zip(groups, saved_groups)):
        raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
    id_map = {old: p for old, p in zip(chain.from_iterable(g["params"] for g in saved_groups), chain.from_iterable(g["params"] for g in groups))}

    def cast(param, value, key=None):
        if isinstance(value, torch.Tensor):
            if key != "step":
                if param.is_floating_point():
                    value = value.to(param.dtype)
                value = value.to(param.device)
            return value
        if isinstance(value, dict):
            return {k: cast(param, v, key=k) for k, v in value.items()}
        if isinstance(value, container_abcs.Iterable) and not isinstance(value, str):
            return type(value)(cast(param, v) for v in value)
        return value

    state = defaultdict(dict)
    for k, v in state_dict["state"].items():
        if k in id_map:
            state[id_map[k]] = cast(id_map[k], v)
        else:
            state[k] = v
    optimizer.__setstate__({"state": state})


def out_dict_to(d: Dict, device=None, code_dtype: torch.dtype = torch.float32, optimizer_dtype: torch.dtype = torch.float32) -> Dict:
    """One cached scene on ``device`` in the cache's storage types (multiscene_nerf.py:17-28)."""
    assert code_dtype.is_floating_point and optimizer_dtype.is_floating_point
    return dict(scene_id=d["scene_id"], scene_name=d["scene_name"],
                param=dict(code_=_clamp_to(d["param"]["code_"], code_dtype).to(device=device, dtype=code_dtype),
                           density_grid=d["param"]["density_grid"].to(device=device),
                           density_bitfield=d["param"]["density_bitfield"].to(device=device)),
                optimizer=optimizer_state_to(d["optimizer"], device=device, dtype=optimizer_dtype))


class _FileWriters:
    """Background ``torch.save`` of cached scenes (the reference forks ``num_file_writers`` processes fed by size-1 queues,
    multiscene_nerf.py:55-72; threads do the same job here - the work is serialisation + file IO, which releases the GIL)."""

    def __init__(self, save_dir: str, n: int):
        self.save_dir = save_dir
        self.queues = [queue.Queue(maxsize=1) for _ in range(n)]
        self.threads = [threading.Thread(target=self._run, args=(q,), daemon=True) for q in self.queues]
        for t in self.threads:
            t.start()
        atexit.register(self.flush)          # daemon threads: make sure queued scenes reach the disk before the interpreter goes away

    def _run(self, q):
        while True:
            obj = q.get()
            try:
                if obj is None:
                    return
                torch.save(obj, os.path.join(self.save_dir, obj["scene_name"] + ".pth"))
            finally:
                q.task_done()

    def put(self, slot: int, obj: Dict):
        self.queues[slot % len(self.queues)].put(obj)

    def flush(self):
        for q in self.queues:
            q.join()


def last_occurrences(scene_ids) -> List[int]:
    """batch rows to keep, in order, when a scene id occurs more than once in a batch: the LAST row of every id (what a loop of per-scene
    writes leaves behind)"""
    last = {int(sid): i for i, sid in enumerate(scene_ids)}
    return sorted(last.values())


CACHE_CAPACITY = 32      # scenes per library call (SSDNERF_CACHE_MAX_SCENES, include/ssdnerf_hip.h); longer batches take several calls
_ADAM_STATE_KEYS = {"step", "exp_avg", "exp_avg_sq"}


class DeviceSceneCache(container_abcs.Mapping):
    """The per-scene training cache held ON THE GPU (``MultiSceneNeRF(cache_store='device')``): one slot per scene of this rank's shard in five
    device arrays -- ``code_`` [N][numel], ``exp_avg`` / ``exp_avg_sq`` [N][numel], ``density_grid`` [N][G^3] fp16, ``density_bitfield`` [N][G^3/8]
    uint8 -- fp32, or fp16 codes and bf16 moments under ``cache_16bit``, allocated on first use.  A training step moves its batch out of the
    slots (``load``) and back (``store``) with ONE launch each (csrc/scene_cache.hip; 32 scenes per launch); values enter a 16-bit store as
    ``_clamp_to(x, dtype).to(dtype)``, bit for bit.  What is not bulk data stays on the host, per slot: ``present`` / ``has_state`` flags,
    Adam's ``step`` (float32), ``scene_id``, ``scene_name`` and the last saved ``param_groups``.

    A read-only ``Mapping`` over the scene ids, like the dict it replaces: ``cache[sid]`` is ``None`` for an empty slot, otherwise the entry of the
    host cache -- same keys, CPU tensors of the same dtypes -- EXPORTED from the slot.  An export is a COPY made at the time of the call (a
    gather and a device-to-host transfer), not a live view: writing to it changes nothing in the cache, and it does not follow later steps.
    ``host_copies`` counts the scenes exported and imported; a training step without ``save_dir`` leaves it unchanged.  ``launches`` counts the
    library calls.  There is no CPU path: ``ensure`` refuses a CPU device."""

    def __init__(self, scene_ids, code_size, grid_size: int, cache_16bit: bool = False):
        self.scene_ids = [int(s) for s in scene_ids]
        self.slot_of = {sid: k for k, sid in enumerate(self.scene_ids)}
        self.code_size = tuple(int(c) for c in code_size)
        self.numel = 1
        for c in self.code_size:
            self.numel *= c
        self.grid_cells = int(grid_size) ** 3
        self.grid_bytes, self.bits_bytes = self.grid_cells * 2, self.grid_cells // 8
        self.code_dtype, self.state_dtype = (torch.float16, torch.bfloat16) if cache_16bit else (torch.float32, torch.float32)
        n = len(self.scene_ids)
        self.present, self.has_state = [False] * n, [False] * n
        self.step: List = [None] * n
        self.scene_id: List = [None] * n
        self.scene_name: List = [None] * n
        self.param_groups: List = [None] * n
        self.host_copies = 0
        self.launches = 0
        self.device = None
        self.code_ = self.exp_avg = self.exp_avg_sq = self.density_grid = self.density_bitfield = None
        self._desc = self._rows = None

    # ---- Mapping ------------------------------------------------------------------------------------------------------------------------------
    def __len__(self):
        return len(self.scene_ids)

    def __iter__(self):
        return iter(self.scene_ids)

    def __getitem__(self, sid):
        slot = self.slot_of[int(sid)]
        return self.export([int(sid)])[0] if self.present[slot] else None

    def slots(self, scene_ids) -> List[int]:
        return [self.slot_of[int(sid)] for sid in scene_ids]

    # ---- device arrays ------------------------------------------------------------------------------------------------------------------------
    def ensure(self, device) -> None:
        """allocate the five arrays on ``device`` at first use (zero-filled)"""
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"cache_store='device' keeps the scene cache on the GPU; the model is on {device} (there is no CPU path)")
        if self.device is not None:
            if device != self.device:
                raise ValueError(f"the scene cache lives on {self.device}, the model is now on {device}")
            return
        from . import _cabi as C
        if C.lib().ssdnerf_cache_max_scenes() != CACHE_CAPACITY:
            raise RuntimeError(f"libssdnerf_hip.so takes {C.lib().ssdnerf_cache_max_scenes()} scenes per cache launch, scene_cache.CACHE_CAPACITY says {CACHE_CAPACITY}: rebuild")
        n = len(self.scene_ids)
        self.code_ = torch.zeros((n, self.numel), dtype=self.code_dtype, device=device)
        self.exp_avg = torch.zeros((n, self.numel), dtype=self.state_dtype, device=device)
        self.exp_avg_sq = torch.zeros((n, self.numel), dtype=self.state_dtype, device=device)
        self.density_grid = torch.zeros((n, self.grid_cells), dtype=torch.float16, device=device)
        self.density_bitfield = torch.zeros((n, self.bits_bytes), dtype=torch.uint8, device=device)
        self.device = device
        half = self.code_dtype == torch.float16
        self._desc = C.CacheStore(self.code_.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.density_grid.data_ptr(),
                                  self.density_bitfield.data_ptr(), n, self.numel, self.grid_bytes, self.bits_bytes, 1 if half else 0, 2 if half else 0)
        self._rows = (C.CacheRow * CACHE_CAPACITY)()

    def _arrays(self):
        return (self.code_, self.exp_avg, self.exp_avg_sq, self.density_grid, self.density_bitfield)

    def _move(self, store: bool, slots: List[int], states: List[bool], leaves, m, v, grid, bits) -> None:
        """``len(slots)`` scenes between the slots and rows 0 .. of the contiguous batch buffers, ``CACHE_CAPACITY`` per launch"""
        from . import _cabi as C
        lib = C.lib()
        fn, what = (lib.ssdnerf_cache_store_multi, "cache_store_multi") if store else (lib.ssdnerf_cache_load_multi, "cache_load_multi")

        def at(t, start, row_bytes):
            return None if t is None else ctypes.c_void_p(t.data_ptr() + start * row_bytes)

        with torch.cuda.device(self.device):
            for start in range(0, len(slots), CACHE_CAPACITY):
                count = min(CACHE_CAPACITY, len(slots) - start)
                any_state = False
                for k in range(count):
                    e = self._rows[k]
                    e.slot, e.row, e.has_state = slots[start + k], k, int(states[start + k])
                    any_state = any_state or states[start + k]
                C.check(fn(self._desc, self._rows, count, at(leaves, start, self.numel * 4), at(m if any_state else None, start, self.numel * 4),
                           at(v if any_state else None, start, self.numel * 4), at(grid, start, self.grid_bytes), at(bits, start, self.bits_bytes),
                           C.stream()), what)
                self.launches += 1
        if store:
            torch.autograd.graph.increment_version(list(self._arrays()))
        else:                # the kernel wrote through raw pointers: tell everything keyed on ``_version``
            torch.autograd.graph.increment_version([t for t in (leaves, m, v, grid, bits) if t is not None])

    def batch_buffers(self, count: int):
        """(leaves, m, v) fp32 (count, *code_size), grid fp16 (count, G^3), bits uint8 (count, G^3/8): uninitialised batch buffers of a step"""
        f = dict(dtype=torch.float32, device=self.device)
        return (torch.empty((count, *self.code_size), **f), torch.empty((count, *self.code_size), **f), torch.empty((count, *self.code_size), **f),
                torch.empty((count, self.grid_cells), dtype=torch.float16, device=self.device),
                torch.empty((count, self.bits_bytes), dtype=torch.uint8, device=self.device))

    def load(self, scene_ids, leaves, m, v, grid, bits) -> None:
        """the slots of ``scene_ids`` (all present; an id may occur twice) into rows 0 .. of the batch buffers, widened to fp32: one launch.  The
        ``m`` / ``v`` rows of slots without optimizer state are left as they are."""
        slots = self.slots(scene_ids)
        if not all(self.present[s] for s in slots):
            raise KeyError(f"DeviceSceneCache.load: empty slots among the scenes {list(scene_ids)}")
        self._check_batch(len(slots), leaves, m, v, grid, bits)
        self._move(False, slots, [self.has_state[s] for s in slots], leaves, m, v, grid, bits)

    def _check_batch(self, count, leaves, m, v, grid, bits):
        for t, dtype, width, name in ((leaves, torch.float32, self.numel, "leaves"), (m, torch.float32, self.numel, "exp_avg"),
                                      (v, torch.float32, self.numel, "exp_avg_sq"), (grid, torch.float16, self.grid_cells, "density_grid"),
                                      (bits, torch.uint8, self.bits_bytes, "density_bitfield")):
            if t is None and name.startswith("exp_avg"):
                continue
            if t.dtype != dtype or t.device != self.device or not t.is_contiguous() or t.numel() != count * width:
                raise ValueError(f"DeviceSceneCache: the {name} batch buffer must be a contiguous {dtype} tensor of {count} x {width} elements on "
                                 f"{self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")

    def _as_rows(self, tensors: List[torch.Tensor]) -> torch.Tensor:
        """a contiguous fp32 (len, numel) buffer whose row j holds ``tensors[j]``: the tensors' own memory when they already are the consecutive
        rows of one (what ``load`` hands out), else gathered into a new one"""
        first = tensors[0]
        stride = self.numel * 4
        if all(t.dtype == torch.float32 and t.device == self.device and t.is_contiguous() and t.numel() == self.numel
               and t.data_ptr() == first.data_ptr() + j * stride for j, t in enumerate(tensors)):
            # one allocation: the consecutive addresses are rows of the same storage, which has to reach past the last of them
            store = first.untyped_storage()
            if all(t.untyped_storage().data_ptr() == store.data_ptr() for t in tensors):
                return torch.as_strided(first.detach(), (len(tensors), self.numel), (self.numel, 1))
        for t in tensors:
            if t.numel() != self.numel:
                raise ValueError(f"DeviceSceneCache: a code or moment of {t.numel()} elements, the cache holds {self.numel} per scene")
        return torch.stack([t.detach().to(device=self.device, dtype=torch.float32).reshape(-1) for t in tensors], dim=0)

    def store(self, scene_ids, scene_names, leaves: List[torch.Tensor], states: List[Dict], param_groups: List, grid: torch.Tensor,
              bits: torch.Tensor) -> List[int]:
        """a batch back into its slots: one launch.  ``states[i]``: ``{}`` or Adam's ``{step, exp_avg, exp_avg_sq}`` of scene i.  Where a scene id
        occurs twice the last occurrence wins (the earlier rows are dropped here, on the host).  -> the batch rows that were stored"""
        keep = last_occurrences(scene_ids)
        for i in keep:
            if states[i] and set(states[i]) != _ADAM_STATE_KEYS:
                raise TypeError(f"DeviceSceneCache holds Adam's optimizer state (step, exp_avg, exp_avg_sq); got the keys {sorted(states[i])} "
                                "(cache_store='host' caches any optimizer)")
        slots = self.slots([scene_ids[i] for i in keep])
        flags = [bool(states[i]) for i in keep]
        rows_l = self._as_rows([leaves[i].data for i in keep])
        rows_m = rows_v = None
        if any(flags):
            zero = None if all(flags) else torch.zeros(self.numel, dtype=torch.float32, device=self.device)
            rows_m = self._as_rows([states[i]["exp_avg"] if states[i] else zero for i in keep])
            rows_v = self._as_rows([states[i]["exp_avg_sq"] if states[i] else zero for i in keep])
        whole = keep == list(range(len(scene_ids)))
        index = None if whole else torch.tensor(keep, device=self.device)
        g = (grid if whole else grid.index_select(0, index.to(grid.device))).to(self.device).contiguous()
        b = (bits if whole else bits.index_select(0, index.to(bits.device))).to(self.device).contiguous()
        self._check_batch(len(keep), rows_l, rows_m, rows_v, g, b)
        self._move(True, slots, flags, rows_l, rows_m, rows_v, g, b)
        for i, slot, flag in zip(keep, slots, flags):
            self.present[slot] = True
            self.scene_id[slot], self.scene_name[slot], self.param_groups[slot] = scene_ids[i], scene_names[i], param_groups[i]
            if flag:
                self.has_state[slot] = True
                self.step[slot] = torch.tensor(float(states[i]["step"]), dtype=torch.float32)
        return keep

    # ---- host copies ---------------------------------------------------------------------------------------------------------------------------
    def export(self, scene_ids) -> List[Optional[Dict]]:
        """the entries of ``scene_ids`` as the host cache holds them (``None`` for empty slots): CPU tensors in the store's dtypes, private copies.
        One gather on the device and one device-to-host transfer for the whole list."""
        slots = self.slots(scene_ids)
        live = [s for s in slots if self.present[s]]
        if not live:
            return [None] * len(slots)
        index = torch.tensor(live, device=self.device)
        packed = torch.cat([a.index_select(0, index).view(torch.uint8).reshape(len(live), -1) for a in self._arrays()], dim=1).cpu()
        self.host_copies += len(live)
        esz, ssz = self.code_.element_size(), self.exp_avg.element_size()
        widths = [self.numel * esz, self.numel * ssz, self.numel * ssz, self.grid_bytes, self.bits_bytes]
        out, r = [], 0
        for sid, slot in zip(scene_ids, slots):
            if not self.present[slot]:
                out.append(None)
                continue
            parts, off = [], 0
            for w in widths:
                parts.append(packed[r, off:off + w].clone())             # (fresh storage: aligned for the dtype view, private to this entry)
                off += w
            r += 1
            entry = dict(scene_id=self.scene_id[slot], scene_name=self.scene_name[slot],
                         param=dict(code_=parts[0].view(self.code_dtype).reshape(self.code_size), density_grid=parts[3].view(torch.float16),
                                    density_bitfield=parts[4]))
            state = {}
            if self.has_state[slot]:
                state[0] = dict(step=self.step[slot].clone(), exp_avg=parts[1].view(self.state_dtype).reshape(self.code_size),
                                exp_avg_sq=parts[2].view(self.state_dtype).reshape(self.code_size))
            if self.param_groups[slot] is not None:
                entry["optimizer"] = dict(state=state, param_groups=self.param_groups[slot])
            out.append(entry)
        return out

    def import_entries(self, entries: Dict[int, Dict], inverse_activation=None) -> None:
        """scene files (``{sid: entry}``, CPU tensors of any float dtype) into their slots, converted by the store's rule: clamp to the target's
        finite range, then round -- where the host cache would keep a loaded tensor's own dtype.  An entry that holds the activated ``code``
        only is inverted by ``inverse_activation`` (with the host path's warning)."""
        import warnings
        sids = list(entries)
        for start in range(0, len(sids), 8):
            part = sids[start:start + 8]
            leaves, states, groups, grids, bitfields = [], [], [], [], []
            for sid in part:
                entry = entries[sid]
                p = entry["param"]
                if "code_" in p:
                    leaf = p["code_"].to(dtype=torch.float32, device=self.device)
                else:
                    warnings.warn("Pre-activation codes not found. Using on-the-fly inversion instead (which could be inconsistent).")
                    leaf = inverse_activation(p["code"].to(dtype=torch.float32, device=self.device))
                leaves.append(leaf)
                opt = entry.get("optimizer")
                if opt is not None and len(opt["state"]) > 1:
                    raise TypeError("DeviceSceneCache: a scene file with more than one optimizer parameter")
                states.append(dict(next(iter(opt["state"].values()))) if opt is not None and opt["state"] else {})
                groups.append(None if opt is None else opt["param_groups"])
                grids.append(p["density_grid"].to(device=self.device, dtype=torch.float16).reshape(-1))
                bitfields.append(p["density_bitfield"].to(device=self.device, dtype=torch.uint8).reshape(-1))
            names = [entries[sid].get("scene_name") for sid in part]
            ids = [entries[sid].get("scene_id", sid) for sid in part]
            self.store(part, names, leaves, states, groups, torch.stack(grids, dim=0), torch.stack(bitfields, dim=0))
            for sid, ident in zip(part, ids):
                self.scene_id[self.slot_of[sid]] = ident
            self.host_copies += len(part)


def read_scene_files(paths: List[str]) -> List[Dict]:
    """``data['code']`` of the reference's dataset (lib/datasets/shapenet_srn.py ``code_dir`` branch): the per-scene dicts, on the CPU."""
    return [torch.load(p, map_location="cpu") for p in paths]
