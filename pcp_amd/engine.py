"""ctypes binding of libpcp_hip.so — the C ABI declared in include/pcp_hip.h.

This is the product path: every call goes through the C-ABI into the hand-written gfx950 kernels.  There is
no CPU fallback: importing works anywhere (so that the non-GPU tests can check the exported symbols), but
``Context()`` raises ``EngineUnavailable`` when the library or a HIP device is missing.
PyTorch is used only as plumbing (device buffers, streams); the ABI itself takes raw pointers.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import inspect
import os
from collections import namedtuple
from typing import Optional

import numpy as np

from .model import PROP_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCP_HIP_LIB", os.path.join(_HERE, "libpcp_hip.so"))  # PCP_HIP_LIB: profiling builds (tools/ablate.sh)

PCP_OK = 0
ERRORS = {-1: "PCP_ERR_ARG", -2: "PCP_ERR_CONTRACT", -3: "PCP_ERR_HIP", -4: "PCP_ERR_NOMEM", -5: "PCP_ERR_UNSUPPORTED", -6: "PCP_ERR_NODEVICE"}

# Every symbol include/pcp_hip.h declares (tests/test_abi.py checks the .so exports each of them).
ABI_SYMBOLS = [
    "pcp_ctx_create", "pcp_ctx_destroy", "pcp_last_error", "pcp_strerror", "pcp_abi_version",
    "pcp_model_reset", "pcp_model_push_props", "pcp_model_push_formula", "pcp_model_push_sum", "pcp_model_truncate", "pcp_model_n_units", "pcp_model_set_hull",
    "pcp_propagate", "pcp_propagate_device", "pcp_propagate_device_units", "pcp_propagate_device_excl", "pcp_propagate_device_small_excl", "pcp_propagate_device_form_excl", "pcp_propagate_device_bnb", "pcp_branch_device", "pcp_branch_device_hint", "pcp_pack_rows", "pcp_unpack_rows", "pcp_branch_device_cells", "pcp_branch_device_set", "pcp_branch_device_set_enum", "pcp_branch_device_excl", "pcp_dfs_device", "pcp_dfs_forest_device", "pcp_dfs_forest_device_form", "pcp_dfs_forest_device_form_bnb", "pcp_dfs_forest_device_small", "pcp_dfs_forest_device_small_bnb", "pcp_dfs_forest_device_small_enum", "pcp_dfs_forest_device_form_enum", "pcp_dfs_forest_device_neq_enum", "pcp_dfs_forest_device_neq_sink", "pcp_dfs_forest_device_set", "pcp_dfs_forest_device_set_enum", "pcp_dfs_forest_device_set_bnb", "pcp_dfs_forest_device_setform", "pcp_dfs_forest_device_setform_bnb", "pcp_dfs_forest_split_set", "pcp_dfs_forest_steal", "pcp_solution_sink_set", "pcp_set_solution_sink_set", "pcp_stats_reset", "pcp_stats_read", "pcp_debug_counters", "pcp_last_kernel_ms", "pcp_last_plan", "pcp_set_option",
]


class PcpStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("steps", "steps3", "narrowings", "waves", "failed_nodes", "nodes", "evaluated", "full_evals")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PcpPlan(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("nodes_per_block", "team", "packed", "word_level", "global_dom", "compact", "implicit_active", "set_mode",
                                          "grid", "block", "lds_bytes", "list_cap", "path")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class DeviceBatch(C.Structure):
    _fields_ = [("lb_in", C.c_void_p), ("ub_in", C.c_void_p), ("lb_out", C.c_void_p), ("ub_out", C.c_void_p),
                ("active_in", C.c_void_p), ("active_out", C.c_void_p), ("status", C.c_void_p), ("bits_in", C.c_void_p), ("bits_out", C.c_void_p),
                ("dirty_var", C.c_void_p), ("cell_format", C.c_uint32), ("reserved", C.c_uint32)]


class Objective(C.Structure):
    """pcp_objective: the objective of pcp_propagate_device_bnb (branch and bound)."""
    _fields_ = [("var", C.c_uint32), ("mode", C.c_uint32), ("best", C.c_void_p), ("best_lb", C.c_void_p), ("best_ub", C.c_void_p),
                ("best_bits", C.c_void_p), ("improved", C.c_void_p), ("reserved", C.c_uint32)]


pcp_objective = Objective
MINIMIZE, MAXIMIZE = 0, 1
VAL_MIDDLE, VAL_MIN = 0, 1  # PCP_VAL_MIDDLE / PCP_VAL_MIN
VAL_MODES = {"middle": VAL_MIDDLE, "min": VAL_MIN}
BOUND_MAX = 0x1FFFFFFF  # PCP_BOUND_MAX
OBJ_MODES = {"min": MINIMIZE, "max": MAXIMIZE}


def no_incumbent(mode) -> int:
    """The `best` of pcp_objective before any solution: PCP_BOUND_MAX + 1 (minimize) or -(PCP_BOUND_MAX + 1) (maximize)."""
    m = OBJ_MODES.get(mode, mode)
    return BOUND_MAX + 1 if m == MINIMIZE else -(BOUND_MAX + 1)


class DfsState(C.Structure):
    _fields_ = [("lb", C.c_void_p), ("ub", C.c_void_p), ("capacity", C.c_uint32), ("sp", C.c_void_p), ("stop", C.c_void_p), ("status", C.c_void_p),
                ("counters", C.c_void_p), ("first_solution", C.c_void_p), ("dirty", C.c_void_p)]


class ForestState(C.Structure):
    _fields_ = [("n_trees", C.c_uint32), ("level_capacity", C.c_uint32), ("trail_capacity", C.c_uint32), ("reserved", C.c_uint32),
                ("bits", C.c_void_p), ("tree", C.c_void_p), ("levels", C.c_void_p), ("trail", C.c_void_p), ("counters", C.c_void_p),
                ("total_nodes", C.c_void_p), ("stop", C.c_void_p), ("first_solution", C.c_void_p), ("solution_flag", C.c_void_p)]


class ForestObjective(C.Structure):
    """pcp_forest_objective: the objective of pcp_dfs_forest_device_set_bnb (branch and bound in the set-mode forest)."""
    _fields_ = [("var", C.c_uint32), ("mode", C.c_uint32), ("best", C.c_void_p), ("tree_best", C.c_void_p), ("tree_row", C.c_void_p)]


class ForestExcl(C.Structure):
    """pcp_forest_excl: the exclusions of pcp_dfs_forest_device_small_enum / _form_enum — one path of entries per tree, two words per stack row."""
    _fields_ = [("path", C.c_void_p), ("row_base", C.c_void_p), ("row_excl", C.c_void_p), ("path_capacity", C.c_uint32), ("val", C.c_uint32)]


class PcpSolutionSink(C.Structure):
    """pcp_solution_sink: the append buffer of (lb, ub) rows the Interval forests write every solution into (pcp_solution_sink_set)."""
    _fields_ = [("lb", C.c_void_p), ("ub", C.c_void_p), ("tree", C.c_void_p), ("count", C.c_void_p), ("capacity", C.c_uint32), ("reserved", C.c_uint32)]


SINK_FULL = 6  # counters[t][3]: the sink was full — the node stays on top of its stack, propagated and uncounted (the contract of error 1)


class SolutionSink:
    """The buffers of a pcp_solution_sink and the host's side of its protocol: ``lb`` / ``ub`` [capacity, n_vars] int32, ``tree`` [capacity]
    int32, ``count`` [1] int32 (torch tensors on ``device``; a CPU device serves the bookkeeping's tests).  ``drain()`` copies the
    min(count, capacity) valid rows to the host — in ticket order, behind what earlier drains brought — and zeroes the count; the copies
    are torch's, on the current stream of the device: the one Context.dfs_forest launches on.  ``rows()`` is everything drained so far."""

    def __init__(self, capacity: int, n_vars: int, device):
        import torch
        if int(capacity) < 1:
            raise ValueError(f"SolutionSink: capacity must be at least 1, not {capacity}")
        self.capacity, self.n_vars = int(capacity), int(n_vars)
        self.lb = torch.zeros((self.capacity, self.n_vars), dtype=torch.int32, device=device)
        self.ub = torch.zeros((self.capacity, self.n_vars), dtype=torch.int32, device=device)
        self.tree = torch.zeros(self.capacity, dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self.drains = 0     # drain() calls
        self.overdrawn = 0  # tickets beyond the capacity, over all drains: the nodes that were handed back
        self._lb, self._ub, self._tree = [], [], []

    def struct(self) -> PcpSolutionSink:
        return PcpSolutionSink(self.lb.data_ptr(), self.ub.data_ptr(), self.tree.data_ptr(), self.count.data_ptr(), self.capacity, 0)

    def drain(self) -> int:
        """Move the valid rows to the host and zero the count.  Returns the number of rows moved."""
        drawn = int(self.count.item()) & 0xFFFFFFFF  # (synchronises: the launches before it have ended)
        n = min(drawn, self.capacity)
        if n:
            self._lb.append(self.lb[:n].cpu().numpy().copy())
            self._ub.append(self.ub[:n].cpu().numpy().copy())
            self._tree.append(self.tree[:n].cpu().numpy().copy())
        self.drains += 1
        self.overdrawn += drawn - n
        self.count.zero_()
        return n

    def rows(self):
        """(lb [n, n_vars], ub [n, n_vars], tree [n]) of every row drained so far, int32 numpy arrays."""
        cat = lambda parts, shape: np.concatenate(parts) if parts else np.zeros(shape, np.int32)
        return cat(self._lb, (0, self.n_vars)), cat(self._ub, (0, self.n_vars)), cat(self._tree, (0,))


class PcpSetSolutionSink(C.Structure):
    """pcp_set_solution_sink: the append buffer of whole nodes (n_vars x set_words words) the set-mode forests write every solution into
    (pcp_set_solution_sink_set)."""
    _fields_ = [("bits", C.c_void_p), ("tree", C.c_void_p), ("count", C.c_void_p), ("capacity", C.c_uint32), ("reserved", C.c_uint32)]


class SetSolutionSink:
    """The buffers of a pcp_set_solution_sink and the host's side of its protocol, as SolutionSink is for the Interval one: ``bits``
    [capacity, n_vars, set_words] int64 (the words of uint64 sets), ``tree`` [capacity] int32, ``count`` [1] int32 (torch tensors on ``device``;
    a CPU device serves the bookkeeping's tests).  ``drain()`` copies the min(count, capacity) valid rows to the host — in ticket order,
    behind what earlier drains brought — and zeroes the count.  ``rows()`` is everything drained so far."""

    def __init__(self, capacity: int, n_vars: int, set_words: int, device):
        import torch
        if int(capacity) < 1:
            raise ValueError(f"SetSolutionSink: capacity must be at least 1, not {capacity}")
        if int(set_words) < 1:
            raise ValueError(f"SetSolutionSink: set_words must be at least 1, not {set_words} (interval-mode stores write into a SolutionSink)")
        self.capacity, self.n_vars, self.set_words = int(capacity), int(n_vars), int(set_words)
        self.bits = torch.zeros((self.capacity, self.n_vars, self.set_words), dtype=torch.int64, device=device)
        self.tree = torch.zeros(self.capacity, dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self.drains = 0     # drain() calls
        self.overdrawn = 0  # tickets beyond the capacity, over all drains: the nodes that were handed back
        self._bits, self._tree = [], []

    def struct(self) -> PcpSetSolutionSink:
        return PcpSetSolutionSink(self.bits.data_ptr(), self.tree.data_ptr(), self.count.data_ptr(), self.capacity, 0)

    def drain(self) -> int:
        """Move the valid rows to the host and zero the count.  Returns the number of rows moved."""
        drawn = int(self.count.item()) & 0xFFFFFFFF  # (synchronises: the launches before it have ended)
        n = min(drawn, self.capacity)
        if n:
            self._bits.append(self.bits[:n].cpu().numpy().view(np.uint64).copy())
            self._tree.append(self.tree[:n].cpu().numpy().copy())
        self.drains += 1
        self.overdrawn += drawn - n
        self.count.zero_()
        return n

    def rows(self):
        """(bits [n, n_vars, set_words] uint64, tree [n] int32) of every row drained so far, numpy arrays."""
        bits = np.concatenate(self._bits) if self._bits else np.zeros((0, self.n_vars, self.set_words), np.uint64)
        return bits, (np.concatenate(self._tree) if self._tree else np.zeros((0,), np.int32))


DFS_FULL = 0xFFFFFFFF


class EngineUnavailable(RuntimeError):
    """libpcp_hip.so is missing or no HIP device is present.  There is deliberately no fallback."""


class PcpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


_lib = None


def load_library():
    """dlopen libpcp_hip.so and declare the prototypes.  Raises EngineUnavailable if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineUnavailable(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")
    # One HIP runtime per process: the PyTorch wheel bundles its own libamdhip64.  If PyTorch is going to be used in
    # this process (device buffers, torch.distributed) its runtime has to be the one that gets loaded, otherwise a
    # later `import torch` finds "No HIP GPUs".  Importing it first makes libpcp_hip.so bind to the same runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:  # missing HIP runtime etc.
        raise EngineUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    L.pcp_abi_version.restype = u32
    L.pcp_strerror.restype = C.c_char_p
    L.pcp_strerror.argtypes = [i32]
    L.pcp_last_error.restype = C.c_char_p
    L.pcp_last_error.argtypes = [vp]
    L.pcp_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.pcp_ctx_destroy.argtypes = [vp]
    L.pcp_ctx_destroy.restype = None
    L.pcp_model_reset.argtypes = [vp, u32, u32]
    L.pcp_model_push_props.argtypes = [vp, u32, vp]
    L.pcp_model_push_sum.argtypes = [vp, u32, vp, C.POINTER(u32)]
    L.pcp_model_push_formula.argtypes = [vp, u32, vp, u32, vp]
    L.pcp_model_push_formula.restype = i32
    L.pcp_model_truncate.argtypes = [vp, u32]
    L.pcp_model_n_units.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.pcp_model_set_hull.argtypes = [vp, i32, i32]
    L.pcp_propagate.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
    L.pcp_propagate_device.argtypes = [vp, u32, C.POINTER(DeviceBatch), vp]
    L.pcp_propagate_device_excl.argtypes = [vp, u32, C.POINTER(DeviceBatch), vp, vp, vp]
    L.pcp_propagate_device_small_excl.argtypes = [vp, u32, C.POINTER(DeviceBatch), vp, vp, C.POINTER(Objective), vp]
    L.pcp_propagate_device_form_excl.argtypes = [vp, u32, C.POINTER(DeviceBatch), vp, vp, C.POINTER(Objective), vp]
    L.pcp_propagate_device_bnb.argtypes = [vp, u32, C.POINTER(DeviceBatch), C.POINTER(Objective), vp]
    L.pcp_branch_device.argtypes = [vp, u32] + [vp] * 9
    L.pcp_branch_device_hint.argtypes = [vp, u32] + [vp] * 10
    L.pcp_pack_rows.argtypes = [vp, u32, vp, vp, vp, vp]
    L.pcp_unpack_rows.argtypes = [vp, u32, vp, vp, vp, vp]
    L.pcp_branch_device_cells.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
    L.pcp_branch_device_set.argtypes = [vp, u32] + [vp] * 9
    L.pcp_branch_device_set_enum.argtypes = [vp, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    L.pcp_branch_device_excl.argtypes = [vp, u32, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, vp, vp]
    L.pcp_dfs_device.argtypes = [vp, C.POINTER(DfsState), u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_set.argtypes = [vp, C.POINTER(ForestState), u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_set_enum.argtypes = [vp, C.POINTER(ForestState), u32, u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_set_bnb.argtypes = [vp, C.POINTER(ForestState), C.POINTER(ForestObjective), u32, u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_setform.argtypes = [vp, C.POINTER(ForestState), u32, u32, u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_setform_bnb.argtypes = [vp, C.POINTER(ForestState), C.POINTER(ForestObjective), u32, u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_split_set.argtypes = [vp, C.POINTER(ForestState), u32, vp, vp, vp]
    L.pcp_dfs_forest_steal.argtypes = [vp, C.POINTER(DfsState), u32, C.POINTER(ForestExcl), u32, vp, vp, vp]
    L.pcp_dfs_forest_device.argtypes = [vp, C.POINTER(DfsState), u32, u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_form.argtypes = [vp, C.POINTER(DfsState), u32, u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_form_bnb.argtypes = [vp, C.POINTER(DfsState), u32, C.POINTER(ForestObjective), u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_small.argtypes = [vp, C.POINTER(DfsState), u32, u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_small_bnb.argtypes = [vp, C.POINTER(DfsState), u32, C.POINTER(ForestObjective), u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_small_enum.argtypes = [vp, C.POINTER(DfsState), u32, C.POINTER(ForestExcl), C.POINTER(ForestObjective), u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_form_enum.argtypes = [vp, C.POINTER(DfsState), u32, C.POINTER(ForestExcl), C.POINTER(ForestObjective), u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_neq_enum.argtypes = [vp, C.POINTER(DfsState), u32, C.POINTER(ForestExcl), C.POINTER(ForestObjective), u32, u32, C.c_uint64, vp]
    L.pcp_dfs_forest_device_neq_sink.argtypes = [vp, C.POINTER(DfsState), u32, C.POINTER(ForestExcl), C.POINTER(PcpSolutionSink), u32, u32, C.c_uint64, vp]
    L.pcp_solution_sink_set.argtypes = [vp, C.POINTER(PcpSolutionSink)]
    L.pcp_set_solution_sink_set.argtypes = [vp, C.POINTER(PcpSetSolutionSink)]
    L.pcp_stats_reset.argtypes = [vp, vp]
    L.pcp_stats_read.argtypes = [vp, C.POINTER(PcpStats), vp]
    L.pcp_debug_counters.argtypes = [vp, C.POINTER(C.c_uint64), u32, vp]
    L.pcp_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.pcp_last_plan.argtypes = [vp, C.POINTER(PcpPlan)]
    L.pcp_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    for f in ("pcp_ctx_create", "pcp_model_reset", "pcp_model_push_props", "pcp_model_push_formula", "pcp_model_push_sum", "pcp_model_truncate", "pcp_model_n_units", "pcp_model_set_hull", "pcp_model_set_hull",
              "pcp_propagate", "pcp_propagate_device", "pcp_propagate_device_units", "pcp_propagate_device_excl", "pcp_propagate_device_small_excl", "pcp_propagate_device_form_excl", "pcp_propagate_device_bnb", "pcp_branch_device", "pcp_branch_device_hint", "pcp_pack_rows", "pcp_unpack_rows", "pcp_branch_device_cells", "pcp_branch_device_set", "pcp_branch_device_set_enum", "pcp_branch_device_excl", "pcp_dfs_device", "pcp_dfs_forest_device", "pcp_dfs_forest_device_form", "pcp_dfs_forest_device_form_bnb", "pcp_dfs_forest_device_small", "pcp_dfs_forest_device_small_bnb", "pcp_dfs_forest_device_small_enum", "pcp_dfs_forest_device_form_enum", "pcp_dfs_forest_device_neq_enum", "pcp_dfs_forest_device_set", "pcp_dfs_forest_device_set_enum", "pcp_dfs_forest_device_set_bnb", "pcp_dfs_forest_device_setform", "pcp_dfs_forest_device_setform_bnb", "pcp_dfs_forest_split_set", "pcp_dfs_forest_steal", "pcp_solution_sink_set", "pcp_set_solution_sink_set", "pcp_stats_reset", "pcp_stats_read", "pcp_debug_counters", "pcp_last_kernel_ms", "pcp_last_plan", "pcp_set_option"):
        getattr(L, f).restype = i32
    _lib = L
    return L


def _np_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _ptr(t):  # the device pointer of a torch tensor (None: a null pointer)
    return None if t is None else C.c_void_p(t.data_ptr())


def _batch(cells=False, **tensors) -> DeviceBatch:
    """pcp_device_batch over torch tensors, by field name (a field not named: a null pointer)."""
    return DeviceBatch(cell_format=1 if cells else 0, **{k: _ptr(t) for k, t in tensors.items()})


def _objective_struct(objective):
    """An Objective from the dict form the propagate_device_* calls take (an Objective or None: itself)."""
    if objective is None or isinstance(objective, Objective):
        return objective
    g = objective.get
    return Objective(int(g("var")), int(OBJ_MODES.get(g("mode"), g("mode"))), _ptr(g("best")), _ptr(g("best_lb")), _ptr(g("best_ub")), _ptr(g("best_bits")),
                     _ptr(g("improved")), 0)

VAR_SELECTS = {"first_smallest": 0, "input_order": 1}  # PCP_VAR_FIRST_SMALLEST / PCP_VAR_INPUT_ORDER: option "var_select" (Context.var_select)


@contextlib.contextmanager
def var_select_scope(ctx, var_select):
    """``ctx.var_select = var_select`` for the duration of the block, the value before restored afterwards — also when the block raises.
    None: the context is not touched at all (no attribute is read, no option set)."""
    if var_select is None:
        yield
        return
    if var_select not in VAR_SELECTS:
        raise ValueError(f"var_select must be 'first_smallest' or 'input_order', not {var_select!r}")
    before = ctx.var_select
    ctx.var_select = var_select
    try:
        yield
    finally:
        ctx.var_select = before


def scoped_var_select(refuse=None):
    """A search driver whose first argument is the context gains the keyword ``var_select=None``: None leaves the context untouched; a name
    of VAR_SELECTS is the context's variable selector for the call (var_select_scope).  ``refuse(arguments)``: a message when the call, as
    bound to the driver's parameters, goes to an entry that selects FirstSmallestVar only — under "input_order" a ValueError."""
    def deco(fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def driver(ctx, *args, var_select=None, **kw):
            if var_select is None:
                return fn(ctx, *args, **kw)
            if var_select not in VAR_SELECTS:
                raise ValueError(f"{fn.__name__}: var_select must be 'first_smallest' or 'input_order', not {var_select!r}")
            if refuse is not None and var_select == "input_order":
                bound = sig.bind(ctx, *args, **kw)
                bound.apply_defaults()
                why = refuse(bound.arguments)
                if why:
                    raise ValueError(f"{fn.__name__}: var_select='input_order' {why}")
            with var_select_scope(ctx, var_select):
                return fn(ctx, *args, **kw)
        driver.__doc__ = (fn.__doc__ or "") + """
        ``var_select`` (keyword; None = the context is left as it is): "first_smallest" or "input_order" — the context's variable selector
        (Context.var_select, option "var_select") for this call, the value before restored afterwards, also when the call raises."""
        return driver
    return deco


def _const_operands(props) -> list:
    """Per filter of a lowered table, the values of its Constant operands (var == PCP_CONST: the value is the operand's offset)."""
    is_const = props["var"] == 0xFFFFFFFF
    return [tuple(int(o) for o, c in zip(off, cst) if c) for off, cst in zip(props["off"], is_const)] if is_const.any() else [()] * len(props)


FOREST_KINDS = (None, "neq", "small", "form")  # dfs_forest_enum / forest_enumerate(forest=): chosen by the store, or one entry forced


def store_forest_kind(ctx) -> str:
    """Context.forest_kind: the Interval forest a store belongs to, decided on the host from its shape — "form" with formula units, "neq" all-XNeqY beyond the small-store limits, else "small"."""
    return "form" if ctx.has_formulas else "neq" if (ctx.all_neq and ctx.beyond_small_limits) else "small"


# One entry point of the Interval forests and what it takes behind ``ctx, st, n_trees``: a pcp_forest_excl, a pcp_forest_objective, a
# pcp_solution_sink, then ``n_steps``, a stop_on_solution word, then ``node_limit, stream``.  dirty: the forest keeps a hint word per stack row.
ForestEntry = namedtuple("ForestEntry", "name excl objective sink stop dirty", defaults=(False, False, False, True, False))


FOREST_ENTRIES = {  # (forest kind, "plain" | "enumerate" | "bnb" | "sink") -> ForestEntry; all-XNeqY stores have no objective to bound: no ("neq", "bnb")
    ("neq", "plain"): ForestEntry("pcp_dfs_forest_device", dirty=True), ("form", "plain"): ForestEntry("pcp_dfs_forest_device_form"),
    ("small", "plain"): ForestEntry("pcp_dfs_forest_device_small"),
    ("form", "bnb"): ForestEntry("pcp_dfs_forest_device_form_bnb", objective=True, stop=False),
    ("small", "bnb"): ForestEntry("pcp_dfs_forest_device_small_bnb", objective=True, stop=False),
    ("neq", "enumerate"): ForestEntry("pcp_dfs_forest_device_neq_enum", excl=True, objective=True, dirty=True),
    ("form", "enumerate"): ForestEntry("pcp_dfs_forest_device_form_enum", excl=True, objective=True),
    ("small", "enumerate"): ForestEntry("pcp_dfs_forest_device_small_enum", excl=True, objective=True),
    ("neq", "sink"): ForestEntry("pcp_dfs_forest_device_neq_sink", excl=True, sink=True, dirty=True)}  # the sink is the call's


def _neq_enum_forest(a, entry=FOREST_ENTRIES["neq", "enumerate"]) -> str:
    """The refusal of dfs_forest_enum / forest_enumerate (forest_solutions: of ``entry``) under InputOrder when the all-XNeqY forest is asked for by name."""
    if a.get("forest") != "neq":
        return ""
    return f"is not served by the all-XNeqY forest ({entry.name} selects FirstSmallestVar only): forest='small' runs an all-XNeqY store within the small-store limits"


def _check_neq_enum(who, objective, collect_solutions, var_select):
    """What the all-XNeqY Enumerate forest (pcp_dfs_forest_device_neq_enum) does not do, raised before anything runs."""
    if objective is not None:
        raise ValueError(f"{who}: there is no branch and bound in the all-XNeqY forest (forest='small' runs one over a store within the small-store limits)")
    if collect_solutions:
        raise ValueError(f"{who}: the all-XNeqY entry behind it refuses the context's solution sink — Context.dfs_forest_neq_solutions / search_forest.forest_solutions return that forest's solutions (forest='small' collects those of a store within the small-store limits)")
    if var_select == "input_order":
        raise ValueError(f"{who}: var_select='input_order' " + _neq_enum_forest({"forest": "neq"}))


def _check_enum_forest(who, ctx, forest, dist, val, objective, collect_solutions, bnb) -> str:
    """What dfs_forest_enum and forest_enumerate refuse, before anything runs; the forest kind — ``forest``, or the store's (None)."""
    if forest not in FOREST_KINDS:
        raise ValueError(f"{who}: forest must be None, 'neq', 'small' or 'form', not {forest!r}")
    if dist is not None:
        raise ValueError(f"{who}: Enumerate does not run on several ranks (moving exclusion lists between ranks is not built)")
    if val not in VAL_MODES:
        raise ValueError(f"{who}: val must be 'middle' or 'min', not {val!r}")
    if collect_solutions and objective is not None:
        raise ValueError(f"{who}: collect_solutions does not go with an objective (branch and bound {bnb})")
    if forest == "neq":
        _check_neq_enum(who, objective, collect_solutions, None)
    if forest is None:
        forest = store_forest_kind(ctx)
    if forest == "neq":
        _check_neq_enum(who, objective, collect_solutions, ctx.var_select)
    return forest


def _xneq_forest(a) -> str:
    """The refusal of dfs_forest / forest_search under InputOrder: neither ``formulas`` nor ``small`` (nor the Enumerate forest chosen by the
    store) is the all-XNeqY in-kernel forest, pcp_dfs_forest_device."""
    if a.get("formulas") or a.get("small"):
        return ""
    return "is not served by the all-XNeqY forest (pcp_dfs_forest_device selects FirstSmallestVar only): small=True runs an all-XNeqY store within the small-store limits"


class Context:
    """One pcp_ctx == one constraint store (CStore) on one GPU."""

    def __init__(self, device: int = 0):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.pcp_ctx_create(device, C.byref(h))
        if rc == -6:
            raise EngineUnavailable("pcp_ctx_create: no HIP device (PCP_ERR_NODEVICE); the engine has no CPU path")
        if rc != 0:
            raise PcpError(rc, self._L.pcp_strerror(rc).decode())
        self._h = h
        self.device = device
        self.n_vars = 0
        self.n_units = 0
        self.set_words = 0
        self._var_select = "first_smallest"
        self.supports_hints = True  # pcp_device_batch.dirty_var / pcp_branch_device_hint (ABI v7): search drivers keep a hint per open node
        self.supports_set_enumerate = True  # pcp_branch_device_set_enum / pcp_dfs_forest_device_set_enum: Enumerate over set-mode stores
        self._neq_flags = []  # per elementary filter pushed: an XNeqY outside a formula with a variable among its operands (all_neq)
        self._form_flags = []  # per elementary filter pushed: a leaf of a formula unit, or a Boolean / BooleanNeg (has_formulas)
        self._const_ops = []  # per elementary filter pushed: the values of its Constant operands (each distinct value is one interned slot: beyond_small_limits)
        for kv in filter(None, os.environ.get("PCP_SET_OPTIONS", "").split(",")):  # experiments: pcp_set_option on every new context (k=v,k=v)
            k_, v_ = kv.split("=")
            self.set_option(k_, int(v_))

    def close(self):
        if getattr(self, "_h", None):
            self._L.pcp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, rc: int):
        if rc != 0:
            raise PcpError(rc, self._L.pcp_last_error(self._h).decode())

    # ---- model ------------------------------------------------------------------------------------------
    def set_model(self, n_vars: int, props: np.ndarray, set_words: int = 0, sums=None):
        """pcp_model_reset + pcp_model_push_props.  set_words > 0: IntervalSet<i32> domains (VStoreSet, the reference's default
        FDSpace) carried as bitsets — declare the hull with set_hull(lo, hi) before propagating (value v = bit v - lo)."""
        props = np.ascontiguousarray(props, dtype=PROP_DTYPE)
        self._check(self._L.pcp_model_reset(self._h, n_vars, int(set_words)))
        self.n_vars = int(n_vars)
        self.set_words = int(set_words)
        self._neq_flags, self._form_flags, self._const_ops = [], [], []
        for members in (sums or []):  # term::Sum views, numbered in order (pcp_model_push_sum)
            mv = np.ascontiguousarray(members, np.uint32)
            t = C.c_uint32()
            self._check(self._L.pcp_model_push_sum(self._h, len(mv), _np_ptr(mv), C.byref(t)))
        self.push_props(props)

    def push_props(self, props: np.ndarray):
        props = np.ascontiguousarray(props, dtype=PROP_DTYPE)
        if len(props):
            self._check(self._L.pcp_model_push_props(self._h, len(props), _np_ptr(props)))
            x, y = props["var"][:, 0].astype(np.int64), props["var"][:, 1].astype(np.int64)
            plain = lambda v: (v < 0xC0000000) | (v == 0xFFFFFFFF)  # a variable or a Constant: no term::Sum view (PCP_SUM)
            self._neq_flags += ((props["kind"] == 0) & plain(x) & plain(y) & ((x < 0xC0000000) | (y < 0xC0000000))).tolist()
            self._form_flags += (props["kind"] >= 7).tolist()  # PCP_BOOL, PCP_NBOOL
            self._const_ops += _const_operands(props)
        self._refresh()

    # ---- the push interface pcp_amd.model.push_model drives (stores with formula propagators) ------------------------------
    def reset_model(self, n_vars: int, set_words: int = 0):
        self._check(self._L.pcp_model_reset(self._h, n_vars, int(set_words)))
        self.n_vars, self.set_words = int(n_vars), int(set_words)
        self._neq_flags, self._form_flags, self._const_ops = [], [], []
        self._refresh()

    def push_sum(self, members) -> int:
        mv = np.ascontiguousarray(members, np.uint32)
        t = C.c_uint32()
        self._check(self._L.pcp_model_push_sum(self._h, len(mv), _np_ptr(mv), C.byref(t)))
        return t.value

    def push_formula(self, nodes: np.ndarray, leaves: np.ndarray):
        """pcp_model_push_formula: ONE unit = a tree of Conjunction / Disjunction nodes over elementary leaves."""
        from .model import FNODE_DTYPE
        nodes = np.ascontiguousarray(nodes, dtype=FNODE_DTYPE)
        leaves = np.ascontiguousarray(leaves, dtype=PROP_DTYPE)
        self._check(self._L.pcp_model_push_formula(self._h, len(nodes), _np_ptr(nodes), len(leaves), _np_ptr(leaves)))
        self._neq_flags += [False] * len(leaves)
        self._form_flags += [True] * len(leaves)
        self._const_ops += _const_operands(leaves)
        self._refresh()

    def set_hull(self, lo: int, hi: int):
        """pcp_model_set_hull: hull of the variables' initial domains (VStore.alloc); forgotten by set_model."""
        self._check(self._L.pcp_model_set_hull(self._h, int(lo), int(hi)))

    def truncate(self, n_units: int):
        self._check(self._L.pcp_model_truncate(self._h, n_units))
        self._refresh()

    def _refresh(self):
        nu, npr = C.c_uint32(), C.c_uint32()
        self._check(self._L.pcp_model_n_units(self._h, C.byref(nu), C.byref(npr)))
        self.n_units, self.n_props = nu.value, npr.value
        self.words = (self.n_units + 63) // 64
        del self._neq_flags[self.n_props:]  # (truncate keeps a prefix of the filters)
        del self._form_flags[self.n_props:]
        del self._const_ops[self.n_props:]

    @property
    def all_neq(self) -> bool:
        """Every elementary filter of the store is a plain XNeqY with a variable among its operands: the models the assignment-driven kernel
        takes (pcp_propagate_device_excl).  The search drivers choose between that entry and pcp_propagate_device_small_excl by it."""
        return bool(self._neq_flags) and len(self._neq_flags) == self.n_props and all(self._neq_flags)

    @property
    def beyond_small_limits(self) -> bool:
        """The store is larger than the small-store kernels take — more than 128 slots (variables and distinct Constant operands) or more
        than 2048 elementary filters: what pcp_dfs_forest_device_small_enum answers with PCP_ERR_UNSUPPORTED, decided here from the store's
        shape so that dfs_forest_enum need not launch to find out."""
        return self.n_vars + len({c for ops in self._const_ops for c in ops}) > 128 or self.n_props > 2048

    @property
    def has_formulas(self) -> bool:
        """The store holds a formula unit or a Boolean / BooleanNeg filter: it runs the tree kernels (last_plan path 3).  The search drivers send
        such a store's Enumerate rounds to pcp_propagate_device_form_excl, every other store's where they went before."""
        return any(self._form_flags)

    forest_kind = property(store_forest_kind)  # "form" | "neq" | "small": the Interval forest dfs_forest_enum / forest_enumerate / forest_solutions choose

    def set_option(self, key: str, value: int):
        self._check(self._L.pcp_set_option(self._h, key.encode(), int(value)))
        if key == "var_select":
            self._var_select = next(k for k, v in VAR_SELECTS.items() if v == int(value))

    @property
    def var_select(self) -> str:
        """The variable selector of every device brancher and search loop (option "var_select"): "first_smallest" (FirstSmallestVar, the
        default) or "input_order" (InputOrder, input_order.rs:30-39: the first variable in store order whose size is > 1).  Under
        "input_order" pcp_dfs_forest_device (the all-XNeqY in-kernel forest) and pcp_branch_device_cells (packed cells) refuse to run."""
        return self._var_select

    @var_select.setter
    def var_select(self, name: str):
        if name not in VAR_SELECTS:
            raise ValueError(f"var_select must be 'first_smallest' or 'input_order', not {name!r}")
        self.set_option("var_select", VAR_SELECTS[name])

    # ---- propagation, host buffers (pcp_propagate) ----------------------------------------------------------
    def propagate_set(self, bits, active: Optional[np.ndarray] = None, want_stats: bool = True):
        """Set mode: ≡ Consistency::consistency on each node's IntervalSet domains.  bits: [n, n_vars, set_words] uint64.
        Returns (lb, ub, bits, active, status, stats) as fresh arrays (lb/ub = the bounds of the fixpoint sets)."""
        bits = np.array(bits, dtype=np.uint64, order="C")
        if bits.ndim == 2:
            bits = bits[None]
        n = bits.shape[0]
        assert bits.shape[1:] == (self.n_vars, self.set_words), bits.shape
        lb = np.zeros((n, self.n_vars), np.int32)
        ub = np.zeros((n, self.n_vars), np.int32)
        if active is not None:
            active = np.array(active, dtype=np.uint64, order="C").reshape(n, self.words)
        status = np.zeros(n, dtype=np.uint8)
        st = PcpStats()
        self._check(self._L.pcp_propagate(self._h, n, _np_ptr(lb), _np_ptr(ub), _np_ptr(bits), _np_ptr(active), _np_ptr(status),
                                          C.byref(st) if want_stats else None))
        return lb, ub, bits, active, status, st.as_dict()

    def propagate(self, lb, ub, active: Optional[np.ndarray] = None, want_stats: bool = True):
        """≡ Consistency::consistency on each row.  Returns (lb, ub, active, status, stats) as fresh arrays."""
        lb = np.array(lb, dtype=np.int32, order="C")
        ub = np.array(ub, dtype=np.int32, order="C")
        n = lb.shape[0] if lb.ndim == 2 else 1
        lb = lb.reshape(n, self.n_vars)
        ub = ub.reshape(n, self.n_vars)
        if active is not None:
            active = np.array(active, dtype=np.uint64, order="C").reshape(n, self.words)
        status = np.zeros(n, dtype=np.uint8)
        st = PcpStats()
        self._check(self._L.pcp_propagate(self._h, n, _np_ptr(lb), _np_ptr(ub), None, _np_ptr(active), _np_ptr(status),
                                          C.byref(st) if want_stats else None))
        return lb, ub, active, status, st.as_dict()

    def propagate_implicit(self, lb, ub, want_active: bool = True, in_place: bool = True):
        """Implicit-active nodes through the device-resident entry: active_in = NULL (every unit active, liveness derived
        from the domains), `active` materialised on request only.  Returns (lb, ub, active or None, status, stats)."""
        import torch
        lb = np.array(lb, dtype=np.int32, order="C")
        n = lb.shape[0] if lb.ndim == 2 else 1
        lb = lb.reshape(n, self.n_vars)
        ub = np.array(ub, dtype=np.int32, order="C").reshape(n, self.n_vars)
        dev = torch.device("cuda", self.device)
        t_lb, t_ub = torch.from_numpy(lb).to(dev), torch.from_numpy(ub).to(dev)
        o_lb, o_ub = (t_lb, t_ub) if in_place else (torch.empty_like(t_lb), torch.empty_like(t_ub))
        t_act = torch.zeros((n, max(self.words, 1)), dtype=torch.int64, device=dev) if want_active else None
        t_st = torch.zeros(n, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        before = self.stats_read(stream)
        self.propagate_device(n, t_lb, t_ub, o_lb, o_ub, None, t_act, t_st, stream)
        after = self.stats_read(stream)
        act = t_act.cpu().numpy().view(np.uint64)[:, : self.words] if want_active else None
        return o_lb.cpu().numpy(), o_ub.cpu().numpy(), act, t_st.cpu().numpy(), {k: after[k] - before[k] for k in after}

    # ---- propagation, device-resident (pcp_propagate_device) ------------------------------------------------
    def propagate_device(self, n_nodes: int, lb_in, ub_in, lb_out, ub_out, active_in, active_out, status, stream_ptr: int = 0,
                         bits_in=None, bits_out=None, dirty=None, cells=False):
        """All arguments are torch tensors on this context's device (or None for the optional masks); nothing is
        synchronised.  Tensors: lb/ub int32 [n,V]; active int64/uint64 [n,words]; status uint8 [n]; set mode: bits int64
        [n,V,set_words] (lb_in/ub_in ignored); dirty int32 [n]: per node the one variable in which it differs from a fixpoint of this
        model, -1 / >= n_vars = none (pcp_device_batch.dirty_var).  cells=True (pcp_device_batch.cell_format PCP_CELLS_PACKED16): lb_in / lb_out
        are int32 [n,V] tensors of packed CELLS (pack_rows), ub_* ignored."""
        bt = _batch(lb_in=lb_in, ub_in=ub_in, lb_out=lb_out, ub_out=ub_out, active_in=active_in, active_out=active_out, status=status,
                    bits_in=bits_in, bits_out=bits_out, dirty_var=dirty, cells=cells)
        self._check(self._L.pcp_propagate_device(self._h, n_nodes, C.byref(bt), C.c_void_p(stream_ptr)))

    def propagate_device_units(self, n_nodes: int, lb_in, ub_in, lb_out, ub_out, active_in, active_out, status, unit_off, units, stream_ptr: int = 0):
        """pcp_propagate_device_units (ABI v8): the batch of `propagate_device` where node i also carries its own unary propagators
        units[unit_off[i] : unit_off[i + 1]] — `unit_off` an int32 device tensor [n + 1], `units` a uint8 device tensor holding the pcp_prop
        records (model.PROP_DTYPE bytes).  Enumerate's x != v children (search/branching/enumerate.rs:48-59) in one launch."""
        bt = _batch(lb_in=lb_in, ub_in=ub_in, lb_out=lb_out, ub_out=ub_out, active_in=active_in, active_out=active_out, status=status)
        self._check(self._L.pcp_propagate_device_units(self._h, n_nodes, C.byref(bt), _ptr(unit_off), _ptr(units), C.c_void_p(stream_ptr)))

    def propagate_device_excl(self, n_nodes: int, lb_in, ub_in, lb_out, ub_out, active_out, status, excl_off, excl, stream_ptr: int = 0, dirty=None):
        """pcp_propagate_device_excl: the batch of `propagate_device` (implicit nodes, int32 rows, an all-XNeqY model on the assignment-driven
        kernel) where node i also carries the value exclusions excl[excl_off[i] : excl_off[i + 1]] — `excl_off` an int32 device tensor [n + 1],
        `excl` an int32 device tensor [m, 2] of (var, value) pairs (the bytes of pcp_excl): Enumerate's x != v right branches
        (search/branching/enumerate.rs:54-59) at any store size that fits LDS.  excl_off = None: exactly propagate_device."""
        bt = _batch(lb_in=lb_in, ub_in=ub_in, lb_out=lb_out, ub_out=ub_out, active_out=active_out, status=status, dirty_var=dirty)
        self._check(self._L.pcp_propagate_device_excl(self._h, n_nodes, C.byref(bt), _ptr(excl_off), _ptr(excl), C.c_void_p(stream_ptr)))

    def propagate_device_small_excl(self, n_nodes: int, lb_in, ub_in, lb_out, ub_out, active_out, status, excl_off, excl, objective=None, stream_ptr: int = 0):
        """pcp_propagate_device_small_excl: the batch of `propagate_device_excl` on a SMALL store of any plain model (at most 128 slots and 2048
        elementary filters, no formula units: the one-wavefront-per-node kernel, last_plan path 4) — node i carries the value exclusions
        excl[excl_off[i] : excl_off[i + 1]] (tensors as in propagate_device_excl; excl_off[0] need not be 0; excl_off = None: no node has any).
        ``objective`` (as in propagate_device_bnb: a dict or an Objective; None: no branch and bound): the incumbent is folded into every
        node's objective cell as the node is staged and the batch's best PCP_TRUE node reduced into it afterwards, all on the device."""
        bt = _batch(lb_in=lb_in, ub_in=ub_in, lb_out=lb_out, ub_out=ub_out, active_out=active_out, status=status)
        ob = _objective_struct(objective)
        self._check(self._L.pcp_propagate_device_small_excl(self._h, n_nodes, C.byref(bt), _ptr(excl_off), _ptr(excl), None if ob is None else C.byref(ob),
                                                            C.c_void_p(stream_ptr)))

    def propagate_device_form_excl(self, n_nodes: int, lb_in, ub_in, lb_out, ub_out, active_out, status, excl_off, excl, objective=None, stream_ptr: int = 0):
        """pcp_propagate_device_form_excl: the batch of `propagate_device_small_excl` on a store WITH formula units (a schedule; four nodes of it
        must fit LDS: the one-wavefront-per-node tree kernel, last_plan path 3) — node i carries the value exclusions
        excl[excl_off[i] : excl_off[i + 1]], swept at the top of every round next to the units (tensors, ``objective`` and the fold / reduce
        as in propagate_device_small_excl; excl_off = None: exactly propagate_device)."""
        bt = _batch(lb_in=lb_in, ub_in=ub_in, lb_out=lb_out, ub_out=ub_out, active_out=active_out, status=status)
        ob = _objective_struct(objective)
        self._check(self._L.pcp_propagate_device_form_excl(self._h, n_nodes, C.byref(bt), _ptr(excl_off), _ptr(excl), None if ob is None else C.byref(ob),
                                                           C.c_void_p(stream_ptr)))

    def propagate_device_bnb(self, n_nodes: int, lb_in, ub_in, lb_out, ub_out, active_in, active_out, status, objective, stream_ptr: int = 0,
                             bits_in=None, bits_out=None):
        """pcp_propagate_device_bnb: `propagate_device` with the incumbent of a branch and bound folded into every node's objective domain
        first and the batch's best PCP_TRUE node reduced into it afterwards, all on the device.  objective: a dict with `var`, `mode`
        ("min" / "max" or MINIMIZE / MAXIMIZE), `best` (int32 [1] tensor) and optionally `best_lb`, `best_ub`, `best_bits`, `improved`
        (int32 tensors [n_vars], int64 [n_vars, set_words], int32 [1]); or an Objective.  No hint (dirty) is taken: nodes are propagated
        from scratch."""
        ob = _objective_struct(objective)
        bt = _batch(lb_in=lb_in, ub_in=ub_in, lb_out=lb_out, ub_out=ub_out, active_in=active_in, active_out=active_out, status=status,
                    bits_in=bits_in, bits_out=bits_out)
        self._check(self._L.pcp_propagate_device_bnb(self._h, n_nodes, C.byref(bt), C.byref(ob), C.c_void_p(stream_ptr)))

    def pack_rows(self, lb, ub, cells=None, stream_ptr: int = 0):
        """pcp_pack_rows: int32 bounds rows [n,V] -> rows of packed cells (an int32 [n,V] tensor whose bits are the cells)."""
        import torch
        if cells is None:
            cells = torch.empty_like(lb)
        self._check(self._L.pcp_pack_rows(self._h, lb.shape[0], C.c_void_p(lb.data_ptr()), C.c_void_p(ub.data_ptr()), C.c_void_p(cells.data_ptr()), C.c_void_p(stream_ptr)))
        return cells

    def unpack_rows(self, cells, lb=None, ub=None, stream_ptr: int = 0):
        """pcp_unpack_rows: rows of packed cells -> (lb, ub) int32 rows."""
        import torch
        lb = torch.empty_like(cells) if lb is None else lb
        ub = torch.empty_like(cells) if ub is None else ub
        self._check(self._L.pcp_unpack_rows(self._h, cells.shape[0], C.c_void_p(cells.data_ptr()), C.c_void_p(lb.data_ptr()), C.c_void_p(ub.data_ptr()), C.c_void_p(stream_ptr)))
        return lb, ub

    def branch_device_cells(self, n_nodes: int, cells, status, child_cells, counts, stream_ptr: int = 0, child_dirty=None):
        """pcp_branch_device_cells: branch_device over rows of packed cells (implicit nodes)."""
        self._check(self._L.pcp_branch_device_cells(self._h, n_nodes, _ptr(cells), _ptr(status), _ptr(child_cells), _ptr(child_dirty), _ptr(counts), C.c_void_p(stream_ptr)))

    def branch_device(self, n_nodes: int, lb, ub, active, status, child_lb, child_ub, child_active, counts, stream_ptr: int = 0, child_dirty=None):
        """pcp_branch_device(_hint) on torch tensors of this context's device (counts: int32[5]; child_dirty: int32 [2 n] capacity, receives
        the variable each child was branched on); nothing is synchronised."""
        self._check(self._L.pcp_branch_device_hint(self._h, n_nodes, _ptr(lb), _ptr(ub), _ptr(active), _ptr(status), _ptr(child_lb), _ptr(child_ub), _ptr(child_active),
                                                   _ptr(child_dirty), _ptr(counts), C.c_void_p(stream_ptr)))

    def branch_device_set(self, n_nodes: int, bits, lb, ub, active, status, child_bits, child_active, counts, stream_ptr: int = 0):
        """pcp_branch_device_set (set mode) on torch tensors of this context's device (counts: int32[5])."""
        self._check(self._L.pcp_branch_device_set(self._h, n_nodes, _ptr(bits), _ptr(lb), _ptr(ub), _ptr(active), _ptr(status), _ptr(child_bits), _ptr(child_active),
                                                  _ptr(counts), C.c_void_p(stream_ptr)))

    def branch_device_set_enum(self, n_nodes: int, bits, lb, ub, active, status, val, child_bits, child_active, counts, stream_ptr: int = 0):
        """pcp_branch_device_set_enum: Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate> over a propagated set-mode batch (rows as for
        branch_device_set).  val: "middle" / "min" (or VAL_MIDDLE / VAL_MIN).  counts: int32[8] = n_children, n_true, n_false, n_unknown,
        n_other, 0, error, 0; an error (3: an Unknown node without a variable of two values or more) is reported there only.  Nothing is
        synchronised; search.branch_enumerate_set is the same brancher on the host and raises instead."""
        self._check(self._L.pcp_branch_device_set_enum(self._h, n_nodes, _ptr(bits), _ptr(lb), _ptr(ub), _ptr(active), _ptr(status), int(VAL_MODES.get(val, val)),
                                                       _ptr(child_bits), _ptr(child_active), _ptr(counts), C.c_void_p(stream_ptr)))

    def branch_device_excl(self, n_nodes: int, lb, ub, status, excl_off, excl, val, child_lb, child_ub, child_excl_off, child_excl, child_excl_capacity: int,
                           counts, stream_ptr: int = 0, child_dirty=None):
        """pcp_branch_device_excl: Brancher<FirstSmallestVar, MiddleVal | MinVal, Enumerate> over a propagated batch whose node i carries the
        exclusions excl[excl_off[i] : excl_off[i + 1]] (int32 device tensors as in propagate_device_excl; excl_off = None: no node has any).
        val: "middle" / "min" (or VAL_MIDDLE / VAL_MIN).  The children's rows go to child_lb / child_ub ([2 n] rows capacity), their lists to
        child_excl ([child_excl_capacity, 2]) with the CSR offsets of the child rows in child_excl_off ([2 n + 1], from 0); counts: int32[8] =
        n_children, n_true, n_false, n_unknown, n_other, n_child_excl, error, 0.  Nothing is synchronised; an error is reported in counts[6]
        only (search.branch_enumerate is the same brancher on the host and raises instead)."""
        self._check(self._L.pcp_branch_device_excl(self._h, n_nodes, _ptr(lb), _ptr(ub), _ptr(status), _ptr(excl_off), _ptr(excl), int(VAL_MODES.get(val, val)), _ptr(child_lb),
                                                   _ptr(child_ub), _ptr(child_dirty), _ptr(child_excl_off), _ptr(child_excl), int(child_excl_capacity), _ptr(counts),
                                                   C.c_void_p(stream_ptr)))

    def dfs_device(self, lb0, ub0, n_steps: int, capacity: int = 4096, stop_on_solution: bool = True, node_limit: int = 0, chunk: int = 256, info: dict | None = None):
        """pcp_dfs_device: the reference's one-node-per-step DFS entirely on the device.  Runs until the stack is empty, a stop
        condition holds or n_steps steps were enqueued (in chunks of `chunk` steps between two reads of the 8-byte state).
        Returns dict(nodes, solutions, failed, error, open, steps_enqueued, first_solution).  ``info`` (a dict) receives ``rows``: the open
        nodes the search left on its stack, (lb, ub) numpy arrays [open, n_vars], bottom row first."""
        import torch
        dev = torch.device("cuda", self.device)
        V = self.n_vars
        lb = torch.zeros((capacity, V), dtype=torch.int32, device=dev)
        ub = torch.zeros((capacity, V), dtype=torch.int32, device=dev)
        lb[0] = torch.from_numpy(np.ascontiguousarray(lb0, np.int32)).to(dev)
        ub[0] = torch.from_numpy(np.ascontiguousarray(ub0, np.int32)).to(dev)
        state = torch.tensor([1, 0], dtype=torch.int32, device=dev)  # sp, stop
        status = torch.zeros(capacity, dtype=torch.uint8, device=dev)
        counters = torch.zeros(5, dtype=torch.int64, device=dev)
        sol = torch.zeros(V, dtype=torch.int32, device=dev)
        dirty = torch.full((capacity,), -1, dtype=torch.int32, device=dev)  # per stack row: the variable it was branched on (the root: none)
        st = DfsState(lb.data_ptr(), ub.data_ptr(), capacity, state.data_ptr(), state.data_ptr() + 4, status.data_ptr(), counters.data_ptr(), sol.data_ptr(), dirty.data_ptr())
        stream = torch.cuda.current_stream(dev).cuda_stream
        done = 0
        while done < n_steps:
            k = min(chunk, n_steps - done)
            self._check(self._L.pcp_dfs_device(self._h, C.byref(st), k, int(bool(stop_on_solution)), int(node_limit), C.c_void_p(stream)))
            done += k
            sp, stop = state.cpu().tolist()
            if sp == 0 or stop:
                break
        cn = counters.cpu().tolist()
        sp, stop = state.cpu().tolist()
        if info is not None:
            info["rows"] = (lb[:sp].cpu().numpy(), ub[:sp].cpu().numpy())
        return {"nodes": cn[0], "solutions": cn[1], "failed": cn[2], "error": cn[3], "open": sp, "stopped": bool(stop), "steps_enqueued": done,
                "first_solution": sol.cpu().numpy() if cn[1] else None}

    def solution_sink_set(self, sink=None):
        """pcp_solution_sink_set: attach a solution sink — a SolutionSink or a PcpSolutionSink over device buffers — to this context, or
        detach the one attached (None).  While one is attached the forests dfs_forest(formulas=True), dfs_forest(small=True) and dfs_forest_enum append every
        solution to it as an (lb, ub) row and hand a node back with error 6 (SINK_FULL) when it is full; every other forest entry refuses to
        run (PCP_ERR_UNSUPPORTED) — the all-XNeqY forest returns its solutions through dfs_forest_neq_solutions, whose sink is the call's.  The struct is copied; the buffers must outlive the attachment."""
        st = sink.struct() if isinstance(sink, SolutionSink) else sink
        self._check(self._L.pcp_solution_sink_set(self._h, None if st is None else C.byref(st)))

    def set_solution_sink_set(self, sink=None):
        """pcp_set_solution_sink_set: attach a set solution sink — a SetSolutionSink or a PcpSetSolutionSink over device buffers — to this
        (set-mode) context, or detach the one attached (None).  While one is attached dfs_forest_set and dfs_forest_setform append every
        solution to it as a whole node and hand a node back with error 6 (SINK_FULL) when it is full; their _bnb drivers' entries refuse to
        run (PCP_ERR_UNSUPPORTED).  The struct is copied; the buffers must outlive the attachment.  set_model (pcp_model_reset) detaches it."""
        st = sink.struct() if isinstance(sink, SetSolutionSink) else sink
        self._check(self._L.pcp_set_solution_sink_set(self._h, None if st is None else C.byref(st)))

    def forest_steal(self, st, n_trees: int, ex, pairs, done, n_pairs=None):
        """pcp_dfs_forest_steal: between two launches of an Interval forest, idle trees take the bottom row of trees with two or more open
        nodes, on the device.  ``st``: the forest's DfsState; ``ex``: its ForestExcl under Enumerate, else None; ``pairs``: [n, 2] int32 device
        tensor of (donor, receiver) trees; ``done``: [n] int32 device tensor, 1 where the pair was valid and carried out.  Enqueued on the
        device's current stream; nothing is read back.  (``n_pairs``: the pair count when it is not ``pairs.shape[0]``.)"""
        import torch
        n = int(pairs.shape[0]) if n_pairs is None else int(n_pairs)
        stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        self._check(self._L.pcp_dfs_forest_steal(self._h, None if st is None else C.byref(st), int(n_trees), None if ex is None else C.byref(ex), n,
                                                 _ptr(pairs), _ptr(done), C.c_void_p(stream)))

    def _run_row_forest(self, entry: ForestEntry, root_lb, root_ub, val, *, root_excl, path_capacity, max_path, stop_on_solution, node_limit_per_tree, steps_per_launch,
                        capacity, max_launches, node_budget, want_solution, rebalance, info, max_capacity, steal, objective=None, sink_mode=None, dist=None, sp0=None,
                        hints=True, sink_capacity=0) -> dict:
        """The host side of every Interval forest, behind dfs_forest, dfs_forest_bnb, dfs_forest_enum and dfs_forest_neq_solutions (which
        validate and choose): the forest's buffers, launches of ``entry`` — marshalled by what the ForestEntry says it takes — through
        search_forest.run_forest_loop, and the result dict.  ``val``: None under BinarySplit, else Enumerate's value selector, and the trees
        carry exclusion paths.  ``objective``: a ForestObjective or None.  ``sink_mode``: None; "context" — a SolutionSink of ``sink_capacity``
        rows is the context's for the duration of the loop, detached on every way out; "call" — it is an argument of every launch."""
        import torch
        from .search_forest import ForestStacks, run_forest_loop
        enum, V = val is not None, self.n_vars
        dev = torch.device("cuda", self.device)
        to_dev = lambda x: (torch.from_numpy(np.ascontiguousarray(x, np.int32)) if isinstance(x, np.ndarray) else x).to(dev).reshape(-1, V)
        rl, ru = to_dev(root_lb), to_dev(root_ub)
        T = rl.shape[0]
        rows = lambda name: ForestStacks.rows(name, T, capacity, V, dev)
        lb, ub = rows("lb"), rows("ub")
        lb[:, 0] = rl; ub[:, 0] = ru
        # (sp0: trees that start with an empty stack — a rank that only takes part in the collectives until a refill reaches it)
        sp = torch.ones(T, dtype=torch.int32, device=dev) if sp0 is None else torch.tensor(list(sp0), dtype=torch.int32, device=dev)
        stop = torch.zeros(T, dtype=torch.int32, device=dev)
        counters = torch.zeros((T, 5), dtype=torch.int64, device=dev)
        sol = torch.zeros((T, V), dtype=torch.int32, device=dev) if want_solution else None
        excl, box = {}, {}  # the Enumerate arrays of the stacks; the structs the launches and the stealer read
        if enum:
            lists = [np.ascontiguousarray(e, np.int32).reshape(-1, 2) for e in root_excl] if root_excl is not None else []
            if lists and len(lists) != T:
                raise ValueError(f"dfs_forest: root_excl names {len(lists)} roots, there are {T}")
            path_capacity = max(int(path_capacity), max((len(e) for e in lists), default=0))
            h_path = np.zeros((T, max(path_capacity, 1), 2), np.int32)
            for t, e in enumerate(lists):
                h_path[t, :len(e)] = e
            excl = dict(path=torch.from_numpy(h_path).to(dev), row_base=rows("row_base"), row_excl=rows("row_excl"), path_capacity=path_capacity,
                        max_path=max(int(max_path), path_capacity))
            if lists:
                excl["row_base"][:, 0] = torch.tensor([len(e) for e in lists], dtype=torch.int32, device=dev)

        def point(fs):  # (re)build the pcp_dfs_state — and the pcp_forest_excl — over the forest's current buffers
            box["st"] = DfsState(fs.lb.data_ptr(), fs.ub.data_ptr(), fs.capacity, sp.data_ptr(), stop.data_ptr(), fs.status.data_ptr(), counters.data_ptr(),
                                 sol.data_ptr() if want_solution else None, fs.dirty.data_ptr() if fs.dirty is not None else None)
            box["ex"] = ForestExcl(fs.path.data_ptr(), fs.row_base.data_ptr(), fs.row_excl.data_ptr(), fs.path_capacity, VAL_MODES[val]) if enum else None

        # pcp_dfs_state.dirty: one word per stack row — the all-XNeqY forest's, under either distributor (the small-store and formula-store forests keep none)
        fs = ForestStacks(lb, ub, rows("status"), sp, stop, counters, max_capacity=max(max_capacity, capacity), on_grow=point,
                          dirty=rows("dirty") if (entry.dirty and hints) else None, **excl)
        del lb, ub, excl
        point(fs)
        fn = getattr(self._L, entry.name)
        stream = torch.cuda.current_stream(dev).cuda_stream
        byref = lambda s: None if s is None else C.byref(s)

        def launch():
            args = [self._h, C.byref(box["st"]), T]
            if entry.excl:
                args.append(byref(box["ex"]))
            if entry.objective:
                args.append(byref(objective))
            if entry.sink:
                args.append(C.byref(box["sink"]))
            args.append(int(steps_per_launch))
            if entry.stop:
                args.append(int(bool(stop_on_solution)))
            self._check(fn(*args, int(node_limit_per_tree), C.c_void_p(stream)))

        sink = SolutionSink(sink_capacity, V, dev) if sink_mode else None
        with contextlib.ExitStack() as on_exit:
            if sink_mode == "context":  # the context's for the duration of the loop only: detached on every way out
                self.solution_sink_set(sink)
                on_exit.callback(self.solution_sink_set, None)
            box["sink"] = sink.struct() if entry.sink else None  # (an argument of every launch: nothing is attached to the context)
            # (the stealer reads the state where point() last put it, so a grown stack or path is the one it moves rows in)
            loop = run_forest_loop(launch, fs, stop_on_solution=stop_on_solution, node_budget=node_budget, rebalance=rebalance and not node_limit_per_tree,
                                   max_launches=max_launches, dist=dist, sink=sink, steal=steal,
                                   stealer=lambda pairs, done: self.forest_steal(box["st"], T, box["ex"], pairs, done))
            if sink is not None:
                sink.drain()  # (behind the last launch)
        if info is not None:
            info.update(loop)
            spc = sp.cpu().tolist()  # the open nodes each tree left on its stack, bottom row first
            info["rows"] = [(fs.lb[t, :spc[t]].cpu().numpy(), fs.ub[t, :spc[t]].cpu().numpy()) for t in range(T)] if T <= 64 else None
            if enum:
                info["path_grown"], info["path_capacity"] = fs.path_grown, fs.path_capacity
        cn = counters.cpu().numpy()
        out = {"nodes": int(cn[:, 0].sum()), "solutions": int(cn[:, 1].sum()), "failed": int(cn[:, 2].sum()), "error": int(cn[:, 3].max()),
               "open": int(sp.sum().item()), "launches": loop["launches"], "per_tree": cn, "trees": T, "steals": loop["steals"],
               "first_solutions": sol.cpu().numpy() if want_solution else None}
        if sink is not None:
            out["solutions_lb"], out["solutions_ub"], out["solution_tree"] = sink.rows()
        return out

    def _run_forest_bnb(self, entry: ForestEntry, root_lb, root_ub, objective, best0, val=None, **run):
        """_run_row_forest under branch and bound: the forest's incumbent (one device word, ``best0`` or "no solution yet") and each tree's
        best value and row, handed to ``entry`` as its pcp_forest_objective; the result gains ``best``, ``best_solution``, ``tree_best``
        (``stop_on_solution`` / ``want_solution`` do not apply)."""
        import torch
        var, mode = objective
        if mode not in OBJ_MODES:
            raise ValueError(f"objective mode must be 'min' or 'max', not {mode!r}")
        none = no_incumbent(mode)
        dev = torch.device("cuda", self.device)
        T = int(np.prod(root_lb.shape)) // max(self.n_vars, 1)
        d_best = torch.full((1,), none if best0 is None else int(best0), dtype=torch.int32, device=dev)
        tree_best = torch.full((T,), none, dtype=torch.int32, device=dev)
        tree_row = torch.zeros((T, self.n_vars), dtype=torch.int32, device=dev)
        obj = ForestObjective(int(var) & 0xFFFFFFFF, OBJ_MODES[mode], d_best.data_ptr(), tree_best.data_ptr(), tree_row.data_ptr())
        out = self._run_row_forest(entry, root_lb, root_ub, val, objective=obj, **{**run, "stop_on_solution": False, "want_solution": False})
        tb = tree_best.cpu().numpy()
        found = tb != none
        out["tree_best"] = tb
        out["best"] = int(d_best.item()) if found.any() else None
        winners = np.nonzero(found & (tb == int(d_best.item())))[0]
        out["best_solution"] = tree_row[int(winners[0])].cpu().numpy() if len(winners) else None
        return out

    @scoped_var_select(refuse=_xneq_forest)
    def dfs_forest(self, root_lb, root_ub, stop_on_solution: bool = False, node_limit_per_tree: int = 0, steps_per_launch: int = 256, capacity: int = 2048,
                   max_launches: int = 1 << 30, node_budget: int = 0, want_solution: bool = False, rebalance: bool = True, info: dict | None = None, dist=None, max_capacity: int = 0,
                   sp0=None, hints: bool = True, formulas: bool = False, small: bool = False, brancher: str = "split", val: str = "middle",
                   root_excl=None, path_capacity: int = 64, max_path: int = 1 << 20, collect_solutions: bool = False, sink_capacity: int = 4096,
                   steal: str = "host"):
        """pcp_dfs_forest_device: the reference's search loop (interval mode, all-XNeqY models) on many subtrees at once, one workgroup per
        tree, each exactly a pcp_dfs_device instance.  root_lb / root_ub: [n_trees, n_vars] int32 (numpy or CUDA tensors): the roots, not yet
        propagated.  Launches of steps_per_launch nodes per tree are repeated until every stack is empty, a tree stopped (solution with
        stop_on_solution / error / its node limit), node_budget nodes were explored by all trees together (checked between launches) or
        max_launches is reached.  With ``dist`` (a torch.distributed group / module, one rank per GPU) the launches run in lockstep on every
        rank, node_budget and the end of the search are GLOBAL (one small all_reduce per launch), and a rank whose trees ran dry takes open
        nodes from the other ranks (search_forest.refill_across_ranks).  ``capacity`` rows per tree are allocated up front and doubled, up to
        ``max_capacity``, whenever a tree fills its stack (error 1 is only reported beyond that).  Returns dict(nodes, solutions, failed, error, open, launches,
        per_tree=[n_trees, 5], first_solutions) — this rank's counters.
        ``formulas``: the store holds formula propagators (Boolean / formula units — what Cumulative.join builds): the trees run in
        pcp_dfs_forest_device_form, one per wavefront (last_plan: path 3, block = 64 x trees per workgroup).  ``small``: a small store of plain
        propagators of any kind (at most 128 slots and 2048 elementary filters, no formula units — the Golomb network): the trees run in
        pcp_dfs_forest_device_small, one per wavefront (last_plan: path 4).  Neither keeps ``dirty`` rows; stacks, growth, refill, ``dist`` and
        the result dict are the same.  Both together are a ValueError: a store is one or the other.
        ``brancher="enumerate"`` (``small=True`` only; otherwise, or with ``dist``, a ValueError; dfs_forest_enum chooses the forest by what the
        store is): the trees run under Enumerate on MiddleVal (``val="middle"``) or MinVal (``"min"``) in pcp_dfs_forest_device_small_enum.
        ``root_excl``: a list of [k, 2] int32 arrays of (var, value), one per root — the exclusions the root arrives with (None: no root has
        any); they are written into each tree's path, which holds ``path_capacity`` entries and is doubled, up to ``max_path``, when a tree
        reports error 5, as its stack is on error 1.  ``info`` also receives ``path_grown`` and ``path_capacity``.
        ``collect_solutions`` (``formulas=True`` or ``small=True``, either brancher, one rank; otherwise a ValueError): every solution is
        returned, not only counted — a SolutionSink of ``sink_capacity`` rows is attached for the duration of the call, a tree that finds it
        full hands its node back (error 6), the loop drains the sink and resumes that tree; the counters are those of the same call without
        it.  The result then also holds ``solutions_lb`` / ``solutions_ub`` ([n, n_vars] int32: a solution is a box of the interval store —
        every point of it satisfies the model; ``first_solutions`` keeps lower bounds only) and ``solution_tree`` ([n]: the tree that wrote
        each row); ``info`` receives ``drains``, the drains a full sink forced.
        ``steal`` ("host" | "device"; anything else a ValueError): how finished trees take work between launches — run_forest_loop's own loop
        over a host copy of ``sp``, or pairs planned on the device (search_forest.plan_steal_pairs) and carried out in one pcp_dfs_forest_steal
        call per launch, with no copy to the host beyond the launch's summary.  Both leave the same state behind, so every tree's counters,
        ``launches`` and ``steals`` are the same.  One rank: "device" with a ``dist`` of more than one rank is a ValueError."""
        _check_steal("dfs_forest", steal, dist)
        if small and formulas:
            raise ValueError("dfs_forest: small=True and formulas=True name two different forests (a store has formula units or it has none)")
        enum = _check_forest_brancher("dfs_forest", brancher, val, small, dist, root_excl)
        _check_collect("dfs_forest", collect_solutions, sink_capacity, small, formulas, dist)
        entry = FOREST_ENTRIES["small" if small else "form" if formulas else "neq", "enumerate" if enum else "plain"]
        return self._run_row_forest(entry, root_lb, root_ub, val if enum else None, sink_mode="context" if collect_solutions else None, root_excl=root_excl,
                                    path_capacity=path_capacity, max_path=max_path, stop_on_solution=stop_on_solution, node_limit_per_tree=node_limit_per_tree, steps_per_launch=steps_per_launch,
                                    capacity=capacity, max_launches=max_launches, node_budget=node_budget, want_solution=want_solution, rebalance=rebalance, info=info, dist=dist,
                                    max_capacity=max_capacity, sp0=sp0, hints=hints, sink_capacity=sink_capacity, steal=steal)

    def dfs_forest_neq_solutions(self, root_lb, root_ub, brancher: str = "split", val: str = "middle", root_excl=None, sink_capacity: int = 4096,
                                 objective=None, var_select=None, dist=None, path_capacity: int = 64, max_path: int = 1 << 20, stop_on_solution: bool = False,
                                 node_limit_per_tree: int = 0, steps_per_launch: int = 256, capacity: int = 2048, max_launches: int = 1 << 30, node_budget: int = 0,
                                 want_solution: bool = False, rebalance: bool = True, info: dict | None = None, max_capacity: int = 0, sp0=None, hints: bool = True,
                                 steal: str = "host"):
        """pcp_dfs_forest_device_neq_sink: every solution of the all-XNeqY in-kernel forest, not only their number — the visitor of AllSolution
        (search/engine/all_solution.rs) on the trees of dfs_forest (``brancher="split"``) or of dfs_forest_enum(forest="neq")
        (``brancher="enumerate"`` on ``val`` "middle" / "min", with ``root_excl`` / ``path_capacity`` / ``max_path`` as there).  It is
        dfs_forest's loop: stacks and paths grow, finished trees steal, and a tree that finds the sink full hands its node back (error 6),
        the loop drains the sink and resumes it.  The sink — a SolutionSink of ``sink_capacity`` rows — is an argument of every launch;
        nothing is attached to the context, whose own sink (solution_sink_set) the all-XNeqY entries keep refusing.  Returns dfs_forest's
        dict plus ``solutions_lb`` / ``solutions_ub`` ([n, n_vars] int32: a solution is a BOX of the interval store, every point of it
        satisfies the model) and ``solution_tree`` ([n]); ``info`` receives ``drains``.  The counters are those of the counting entry on
        the same roots.  An ``objective`` (there is no branch and bound in this forest), ``var_select="input_order"`` (given, or the
        context's), ``sink_capacity`` < 1 and a ``dist`` are a ValueError before anything runs.  ``steal``: as for dfs_forest."""
        who = "dfs_forest_neq_solutions"
        _check_brancher(brancher, val)
        _check_steal(who, steal, dist)
        if objective is not None:
            raise ValueError(f"{who}: there is no branch and bound in the all-XNeqY forest (dfs_forest_bnb(small=True) runs one over a store within the small-store limits)")
        if var_select is not None and var_select not in VAR_SELECTS:
            raise ValueError(f"{who}: var_select must be 'first_smallest' or 'input_order', not {var_select!r}")
        if var_select == "input_order":
            raise ValueError(f"{who}: var_select='input_order' is not served by the all-XNeqY forest (pcp_dfs_forest_device_neq_sink selects FirstSmallestVar only): "
                             "dfs_forest(small=True, collect_solutions=True) runs an all-XNeqY store within the small-store limits")
        if int(sink_capacity) < 1:
            raise ValueError(f"{who}: sink_capacity must be at least 1, not {sink_capacity}")
        if dist is not None:
            raise ValueError(f"{who}: collecting solutions does not run on several ranks (gathering the sinks is not built)")
        if root_excl is not None and brancher != "enumerate":
            raise ValueError(f"{who}: root_excl needs brancher='enumerate'")
        with var_select_scope(self, var_select):
            if self.var_select == "input_order":
                raise ValueError(f"{who}: the context's var_select is 'input_order', which the all-XNeqY forest does not serve (var_select='first_smallest' for this call)")
            return self._run_row_forest(FOREST_ENTRIES["neq", "sink"], root_lb, root_ub, val if brancher == "enumerate" else None, sink_mode="call",
                                        root_excl=root_excl, path_capacity=path_capacity, max_path=max_path, stop_on_solution=stop_on_solution, node_limit_per_tree=node_limit_per_tree,
                                        steps_per_launch=steps_per_launch, capacity=capacity, max_launches=max_launches, node_budget=node_budget, want_solution=want_solution,
                                        rebalance=rebalance, info=info, max_capacity=max_capacity, sp0=sp0, hints=hints, sink_capacity=sink_capacity, steal=steal)

    @scoped_var_select()
    def dfs_forest_bnb(self, root_lb, root_ub, objective, best0=None, node_limit_per_tree: int = 0, steps_per_launch: int = 256, capacity: int = 2048,
                       max_launches: int = 1 << 30, node_budget: int = 0, rebalance: bool = True, info: dict | None = None, dist=None, max_capacity: int = 0,
                       sp0=None, small: bool = False, brancher: str = "split", val: str = "middle", root_excl=None, path_capacity: int = 64,
                       max_path: int = 1 << 20, collect_solutions: bool = False, steal: str = "host"):
        """pcp_dfs_forest_device_form_bnb: branch and bound (branch_and_bound.rs:64-84) in the forest over an Interval store with formula
        propagators — the loop, stacks, growth and refill of dfs_forest(formulas=True), every popped row entered with the forest's incumbent
        (one device word) folded into the objective's bounds.  ``objective`` = (var, "min" | "max").  ``best0``: a known bound to start from
        (only solutions that beat it are found).  Returns the dict of dfs_forest plus ``best`` (None: no tree found a solution),
        ``best_solution`` (the row of the lowest tree whose value is ``best``) and ``tree_best`` ([n_trees]; a tree without a solution: the
        "no solution yet" value).
        ``small``: the store is a small one of plain propagators (dfs_forest(small=True)): the same loop and result over
        pcp_dfs_forest_device_small_bnb.  ``brancher`` / ``val`` / ``root_excl`` / ``path_capacity`` / ``max_path``: as for dfs_forest
        (Enumerate needs ``small=True``: pcp_dfs_forest_device_small_enum with the objective — the bnb entry is not called then;
        dfs_forest_enum(objective=) runs it over either store).  ``collect_solutions=True`` is a ValueError:
        branch and bound keeps ``best_solution``, and its entries refuse a solution sink.  ``steal``: as for dfs_forest (the per-tree
        branch-and-bound words stay with their trees under both)."""
        _check_steal("dfs_forest_bnb", steal, dist)
        enum = _check_forest_brancher("dfs_forest_bnb", brancher, val, small, dist, root_excl)
        _check_collect("dfs_forest_bnb", collect_solutions, 1, small, not small, None, bnb=True)
        entry = FOREST_ENTRIES["small" if small else "form", "enumerate" if enum else "bnb"]
        return self._run_forest_bnb(entry, root_lb, root_ub, objective, best0, val if enum else None, root_excl=root_excl, path_capacity=path_capacity, max_path=max_path,
                                    node_limit_per_tree=node_limit_per_tree, steps_per_launch=steps_per_launch, capacity=capacity, max_launches=max_launches,
                                    node_budget=node_budget, rebalance=rebalance, info=info, dist=dist, max_capacity=max_capacity, sp0=sp0, steal=steal)

    @scoped_var_select(refuse=_neq_enum_forest)
    def dfs_forest_enum(self, root_lb, root_ub, val: str = "middle", objective=None, best0=None, root_excl=None, path_capacity: int = 64, max_path: int = 1 << 20,
                        collect_solutions: bool = False, sink_capacity: int = 4096, stop_on_solution: bool = False, node_limit_per_tree: int = 0,
                        steps_per_launch: int = 256, capacity: int = 2048, max_launches: int = 1 << 30, node_budget: int = 0, want_solution: bool = False,
                        rebalance: bool = True, info: dict | None = None, dist=None, max_capacity: int = 0, forest=None, hints: bool = True, steal: str = "host"):
        """The Enumerate forest over this context's Interval store, chosen by what the store IS (as search.dfs_enumerate and DeviceSearch
        dispatch): pcp_dfs_forest_device_form_enum when it holds formula units (``has_formulas`` — schedules, what Cumulative.join builds),
        else pcp_dfs_forest_device_small_enum.  The trees run under Enumerate on MiddleVal (``val="middle"``) or MinVal (``"min"``); roots,
        ``root_excl``, ``path_capacity`` / ``max_path``, ``collect_solutions`` / ``sink_capacity``, the loop keywords, stack and path growth,
        steals and the result dict are those of dfs_forest(brancher="enumerate") — it is that loop.  ``objective`` = (var, "min" | "max"):
        under branch and bound, ``best0`` a known bound to start from; the result then also holds the keys of dfs_forest_bnb (``best``,
        ``best_solution``, ``tree_best``), and ``stop_on_solution`` / ``want_solution`` do not apply.  One rank: ``dist`` is a ValueError,
        as are a ``val`` other than "middle" / "min", ``collect_solutions`` with an objective, and a ``root_excl`` whose length is not the
        number of roots.
        ``forest`` (None / "neq" / "small" / "form"; anything else a ValueError): None chooses by the store (``forest_kind``); a name forces
        that entry.  "neq" is the all-XNeqY in-kernel forest, pcp_dfs_forest_device_neq_enum: one workgroup per tree, any all-XNeqY store the
        in-kernel search takes (N-queens-1000; forced, small N-queens too), the stack rows with their ``dirty`` words (``hints=False``: without
        them — the same tree).  It has no branch and bound, refuses the context's solution sink (dfs_forest_neq_solutions returns its solutions)
        and selects FirstSmallestVar only: ``objective``, ``collect_solutions`` and ``var_select="input_order"`` are a ValueError before anything runs.
        ``steal``: as for dfs_forest; a stolen row takes its ``dirty``, ``row_base`` / ``row_excl`` words and its path prefix along under both."""
        _check_steal("dfs_forest_enum", steal, dist)
        forest = _check_enum_forest("dfs_forest_enum", self, forest, dist, val, objective, collect_solutions, "keeps best_solution; its entries refuse a solution sink")
        entry = FOREST_ENTRIES[forest, "enumerate"]
        run = dict(root_excl=root_excl, path_capacity=path_capacity, max_path=max_path, node_limit_per_tree=node_limit_per_tree, steps_per_launch=steps_per_launch,
                   capacity=capacity, max_launches=max_launches, node_budget=node_budget, rebalance=rebalance, info=info, max_capacity=max_capacity, hints=hints, steal=steal)
        if objective is not None:
            return self._run_forest_bnb(entry, root_lb, root_ub, objective, best0, val, **run)
        _check_collect("dfs_forest", collect_solutions, sink_capacity, forest == "small", forest == "form", None)
        return self._run_row_forest(entry, root_lb, root_ub, val, sink_mode="context" if collect_solutions else None, stop_on_solution=stop_on_solution,
                                    want_solution=want_solution, sink_capacity=sink_capacity, **run)

    @scoped_var_select()
    def dfs_forest_set(self, root_bits, stop_on_solution: bool = False, node_limit: int = 0, steps_per_launch: int = 256,
                       level_capacity: int = 0, trail_capacity: int = 0, max_launches: int = 1 << 30, want_solution: bool = True,
                       info: dict | None = None, rebalance: bool = True, brancher: str = "split", val: str = "middle",
                       collect_solutions: bool = False, sink_capacity: int = 4096):
        """pcp_dfs_forest_device_set: the reference's search loop over FDSpace on the device, one tree per workgroup, the current
        node in LDS, an undo trail in HBM.  brancher="enumerate": the same loop under Enumerate on MiddleVal (val="middle") or MinVal ("min"),
        pcp_dfs_forest_device_set_enum; val is ignored under "split" (BinarySplit on MiddleVal).  root_bits: [n_trees, n_vars, set_words] uint64 (numpy or a CUDA int64 tensor): the roots,
        not yet propagated.  Launches of steps_per_launch nodes per tree are repeated until every tree is finished, the forest
        stopped (solution / node limit / error) or max_launches is reached.
        Returns dict(nodes, solutions, failed, error, finished_trees, stopped, launches, first_solution, per_tree=[n_trees, 4]).
        ``collect_solutions``: every solution is returned, not only counted — a SetSolutionSink of ``sink_capacity`` rows is attached for the
        duration of the call, a tree that finds it full hands its node back (error 6), the loop drains the sink and resumes; the counters
        are those of the same call without it.  The result then also holds ``solutions_bits`` ([n, n_vars, set_words] uint64: a solution is
        a product of sets — every point of it satisfies the model; ``first_solution`` keeps lower bounds only) and ``solution_tree`` ([n]:
        the tree that wrote each row); ``info`` receives ``drains`` and ``handed_back``.  With the default False the calls issued and the
        keys returned are those of before."""
        _check_brancher(brancher, val)
        _check_collect_set("dfs_forest_set", collect_solutions, sink_capacity)

        def launch(st, steps, stream):
            if brancher == "enumerate":
                return self._L.pcp_dfs_forest_device_set_enum(self._h, C.byref(st), VAL_MODES[val], steps, int(bool(stop_on_solution)), int(node_limit), C.c_void_p(stream))
            return self._L.pcp_dfs_forest_device_set(self._h, C.byref(st), steps, int(bool(stop_on_solution)), int(node_limit), C.c_void_p(stream))

        return self._run_forest_set(root_bits, launch, node_limit=node_limit, steps_per_launch=steps_per_launch, level_capacity=level_capacity,
                                    trail_capacity=trail_capacity, max_launches=max_launches, want_solution=want_solution, info=info, rebalance=rebalance,
                                    **(dict(collect=int(sink_capacity), stop_on_solution=stop_on_solution) if collect_solutions else {}))

    @scoped_var_select()
    def dfs_forest_setform(self, root_bits, stop_on_solution: bool = False, node_limit: int = 0, steps_per_launch: int = 256,
                           level_capacity: int = 0, trail_capacity: int = 0, max_launches: int = 1 << 30, want_solution: bool = True,
                           info: dict | None = None, rebalance: bool = True, brancher: str = "split", val: str = "middle",
                           collect_solutions: bool = False, sink_capacity: int = 4096):
        """pcp_dfs_forest_device_setform: dfs_forest_set for a store WITH formula propagators (Boolean / formula units) — the same loop, state
        and result dict, one tree per wavefront with its node in a slice of a CU's LDS (last_plan: block = 64 x trees per workgroup, path 3).
        A store without formula propagators raises PCP_ERR_UNSUPPORTED (dfs_forest_set searches it), as dfs_forest_set does for one with.
        ``collect_solutions`` / ``sink_capacity``: as for dfs_forest_set."""
        _check_brancher(brancher, val)
        _check_collect_set("dfs_forest_setform", collect_solutions, sink_capacity)

        def launch(st, steps, stream):
            return self._L.pcp_dfs_forest_device_setform(self._h, C.byref(st), 1 if brancher == "enumerate" else 0, VAL_MODES.get(val, VAL_MIDDLE), steps,
                                                         int(bool(stop_on_solution)), int(node_limit), C.c_void_p(stream))

        return self._run_forest_set(root_bits, launch, node_limit=node_limit, steps_per_launch=steps_per_launch, level_capacity=level_capacity,
                                    trail_capacity=trail_capacity, max_launches=max_launches, want_solution=want_solution, info=info, rebalance=rebalance,
                                    **(dict(collect=int(sink_capacity), stop_on_solution=stop_on_solution) if collect_solutions else {}))

    def _run_forest_set(self, root_bits, launch, node_limit: int = 0, steps_per_launch: int = 256, level_capacity: int = 0, trail_capacity: int = 0,
                        max_launches: int = 1 << 30, want_solution: bool = False, info: dict | None = None, rebalance: bool = True, live=None,
                        ramp_steps: int = 0, collect: int = 0, stop_on_solution: bool = False, _sink=None):
        """The host side of the set-mode forest, shared by dfs_forest_set and dfs_forest_set_bnb: the forest's buffers, then launches of
        ``launch(st, steps, stream)`` (a pcp_dfs_forest_device_set* call, its return code) until every tree is finished, the forest stopped or
        max_launches is reached; between launches finished trees take work through pcp_dfs_forest_split_set.  ``live`` ([n_trees] bool or
        None = all): the trees that start with a root; the others start finished and only receive work.  ``ramp_steps`` > 0: launches of that
        many nodes while trees are still idle at the start, so that the splits fill them (at most 2 log2(n_trees) + 4 such launches).
        ``collect`` > 0 (with the caller's ``stop_on_solution``): a SetSolutionSink of that many rows is attached for the loop and detached
        on every way out.  In this forest ``stop`` is ONE word for all trees, so after a launch the trees with error 6 are handed back — the
        sink drained, their error word zeroed — and the stop word is cleared and the loop resumes only when error 6 is the SOLE cause of the
        stop: no tree holds another error, the node limit is not reached, and no solution was counted under stop_on_solution.  Otherwise the
        search ends as it would have, the handed-back nodes being uncounted open nodes of a stopped forest, and ``error`` reports the other
        cause, or 0.  Returns the result dict of dfs_forest_set."""
        import torch
        dev = torch.device("cuda", self.device)
        V, sw = self.n_vars, self.set_words
        if collect:
            sink = SetSolutionSink(collect, V, sw, dev)
            self.set_solution_sink_set(sink)
            try:
                out = self._run_forest_set(root_bits, launch, node_limit=node_limit, steps_per_launch=steps_per_launch, level_capacity=level_capacity,
                                           trail_capacity=trail_capacity, max_launches=max_launches, want_solution=want_solution, info=info,
                                           rebalance=rebalance, live=live, ramp_steps=ramp_steps, stop_on_solution=stop_on_solution, _sink=sink)
                sink.drain()
            finally:
                self.set_solution_sink_set(None)
            out["solutions_bits"], out["solution_tree"] = sink.rows()
            return out
        # 0 = the model's own bound: a trail entry takes at least one value out of a set and is popped before the value can return, so a
        # tree never holds more entries (or open levels) than the root has values
        bound = V * sw * 64 + 16
        trail_capacity = int(trail_capacity) or bound
        level_capacity = int(level_capacity) or min(bound, 1 << 14)
        if isinstance(root_bits, np.ndarray):
            bits = torch.from_numpy(np.ascontiguousarray(root_bits).view(np.int64)).to(dev)
        else:
            bits = root_bits.to(dev).contiguous().clone()
        bits = bits.reshape(-1, V, sw)
        T = bits.shape[0]
        tree = torch.zeros((T, 4), dtype=torch.int32, device=dev)
        tree[:, 2] = -1  # PCP_DFS_FULL
        if live is not None:
            tree[:, 3] = torch.from_numpy(1 - np.asarray(live, bool).astype(np.int32).reshape(T)).to(dev)  # finished: nothing of its own
        levels = torch.empty((T, level_capacity, 4), dtype=torch.int32, device=dev)  # (written before they are read: no fill)
        trail = torch.empty((T, trail_capacity, 4), dtype=torch.int32, device=dev)
        counters = torch.zeros((T, 4), dtype=torch.int64, device=dev)
        glob = torch.zeros(4, dtype=torch.int64, device=dev)  # total nodes | stop (low word of [1]) | solution flag (low word of [2])
        sol = torch.zeros(V, dtype=torch.int32, device=dev) if want_solution else None
        st = ForestState(T, level_capacity, trail_capacity, 0, bits.data_ptr(), tree.data_ptr(), levels.data_ptr(), trail.data_ptr(), counters.data_ptr(),
                         glob.data_ptr(), glob.data_ptr() + 8, sol.data_ptr() if want_solution else None, glob.data_ptr() + 16 if want_solution else None)
        stream = torch.cuda.current_stream(dev).cuda_stream
        launches = splits = handed_back = 0
        ramp_left = (2 * max(T - 1, 1).bit_length() + 4) if ramp_steps else 0
        while launches < max_launches:
            self._check(launch(st, int(ramp_steps) if ramp_left else int(steps_per_launch), stream))
            launches += 1
            g = glob.cpu().tolist()  # (the launch's only synchronisation)
            ts = tree.cpu().numpy()
            fin = (ts[:, 3] & 1) != 0
            if _sink is not None and (g[1] & 0xFFFFFFFF):
                cn = counters.cpu().numpy()
                full = cn[:, 3] == SINK_FULL
                if full.any():
                    # hand the nodes back: the rows out, those trees' error word zeroed; resume only if nothing else stopped the forest
                    _sink.drain()
                    handed_back += int(full.sum())
                    counters[torch.from_numpy(full).to(dev), 3] = 0
                    other = (cn[~full, 3] != 0).any() or (node_limit and g[0] >= node_limit) or (stop_on_solution and cn[:, 1].sum() > 0)
                    if not other:
                        glob[1] = 0
                        g[1] = 0
            if (g[1] & 0xFFFFFFFF) or (node_limit and g[0] >= node_limit) or fin.all():
                break
            ramp_left = ramp_left - 1 if (ramp_left and fin.any()) else 0
            if rebalance and fin.any():
                # finished trees take the oldest open right branch of the trees with the most levels left (pcp_dfs_forest_split_set)
                left = np.where(fin, 0, ts[:, 0].astype(np.int64) - (ts[:, 3] >> 8))
                donors = [int(i) for i in np.argsort(-left) if left[i] > 0]
                recv = [int(i) for i in np.nonzero(fin)[0]]
                k = min(len(donors), len(recv))
                if k:
                    pairs = torch.tensor(np.stack([donors[:k], recv[:k]], axis=1).astype(np.int32).ravel(), dtype=torch.int32, device=dev)
                    done = torch.zeros(k, dtype=torch.int32, device=dev)
                    self._check(self._L.pcp_dfs_forest_split_set(self._h, C.byref(st), k, C.c_void_p(pairs.data_ptr()), C.c_void_p(done.data_ptr()), C.c_void_p(stream)))
                    splits += int(done.sum().item())
        cn = counters.cpu().numpy()
        g = glob.cpu().tolist()
        if info is not None:
            info.update(trail_max=int(tree[:, 1].max().item()), levels_max=int(tree[:, 0].max().item()), trees=T, splits=splits)
            if _sink is not None:
                info.update(drains=_sink.drains, handed_back=handed_back, overdrawn=_sink.overdrawn)  # (equal: a ticket beyond the capacity is a node handed back)
        return {"nodes": int(cn[:, 0].sum()), "solutions": int(cn[:, 1].sum()), "failed": int(cn[:, 2].sum()), "error": int(cn[:, 3].max()),
                "finished_trees": int((tree[:, 3] & 1).sum().item()), "splits": splits, "stopped": bool(g[1] & 0xFFFFFFFF), "launches": launches, "total_nodes": int(g[0]),
                "first_solution": sol.cpu().numpy() if (want_solution and (g[2] & 0xFFFFFFFF)) else None, "per_tree": cn}

    @scoped_var_select()
    def dfs_forest_set_bnb(self, root_bits, objective, live=None, best0=None, brancher: str = "split", val: str = "middle", steps_per_launch: int = 256,
                           node_limit: int = 0, level_capacity: int = 0, trail_capacity: int = 0, rebalance: bool = True, info: dict | None = None,
                           ramp_steps: int = 0, max_launches: int = 1 << 30, collect_solutions: bool = False, formulas: bool = False):
        """pcp_dfs_forest_device_set_bnb: branch and bound (branch_and_bound.rs:64-84) in the set-mode forest — the loop of dfs_forest_set under
        either ``brancher``, every node entered with the forest's incumbent (one device word) folded into the set of the objective variable.
        ``objective`` = (var, "min" | "max").  ``live``: which trees start with a root ([n_trees] bool; None: all); the others start finished
        and receive work through pcp_dfs_forest_split_set.  ``best0``: a known bound to start from (only solutions that beat it are found).
        ``ramp_steps``: see _run_forest_set.  Returns the counters of dfs_forest_set (first_solution: None) plus ``best`` (None: no solution and
        no ``best0``), ``best_solution`` (the row of the lowest tree whose value is ``best``; None when no tree found one) and ``tree_best`` ([n_trees], a tree
        without a solution: the "no solution yet" value).  ``collect_solutions=True`` is a ValueError: branch and bound keeps
        ``best_solution``, and its entries refuse a set solution sink.  ``formulas``: pcp_dfs_forest_device_setform_bnb (dfs_forest_setform_bnb)."""
        who, entry = ("dfs_forest_setform_bnb", "pcp_dfs_forest_device_setform_bnb") if formulas else ("dfs_forest_set_bnb", "pcp_dfs_forest_device_set_bnb")
        import torch
        _check_brancher(brancher, val)
        _check_collect_set(who, collect_solutions, 1, bnb=True)
        var, mode = objective
        if mode not in OBJ_MODES:
            raise ValueError(f"objective mode must be 'min' or 'max', not {mode!r}")
        if not 0 <= int(var) < self.n_vars:
            raise ValueError(f"objective variable {var} out of range")
        none = no_incumbent(mode)
        dev = torch.device("cuda", self.device)
        T = int(np.prod(root_bits.shape)) // (self.n_vars * self.set_words)
        d_best = torch.full((1,), none if best0 is None else int(best0), dtype=torch.int32, device=dev)
        tree_best = torch.full((T,), none, dtype=torch.int32, device=dev)
        tree_row = torch.zeros((T, self.n_vars), dtype=torch.int32, device=dev)
        obj = ForestObjective(int(var), OBJ_MODES[mode], d_best.data_ptr(), tree_best.data_ptr(), tree_row.data_ptr())

        def launch(st, steps, stream):
            return getattr(self._L, entry)(self._h, C.byref(st), C.byref(obj), 1 if brancher == "enumerate" else 0, VAL_MODES.get(val, VAL_MIDDLE), steps,
                                            int(node_limit), C.c_void_p(stream))

        out = self._run_forest_set(root_bits, launch, node_limit=node_limit, steps_per_launch=steps_per_launch, level_capacity=level_capacity,
                                   trail_capacity=trail_capacity, max_launches=max_launches, info=info, rebalance=rebalance, live=live, ramp_steps=ramp_steps)
        best = int(d_best.item())
        tb = tree_best.cpu().numpy()
        winners = np.nonzero(tb == best)[0] if best != none else []
        out["tree_best"] = tb
        out["best"] = None if best == none else best  # (a seeded incumbent nothing beat stays the best known value)
        out["best_solution"] = tree_row[int(winners[0])].cpu().numpy() if len(winners) else None
        return out

    @scoped_var_select()
    def dfs_forest_setform_bnb(self, root_bits, objective, **kw):
        """pcp_dfs_forest_device_setform_bnb: dfs_forest_set_bnb for a store WITH formula propagators (see dfs_forest_setform) — the same
        arguments and result dict."""
        return self.dfs_forest_set_bnb(root_bits, objective, formulas=True, **kw)

    def stats_reset(self, stream_ptr: int = 0):
        self._check(self._L.pcp_stats_reset(self._h, C.c_void_p(stream_ptr)))

    def stats_read(self, stream_ptr: int = 0) -> dict:
        st = PcpStats()
        self._check(self._L.pcp_stats_read(self._h, C.byref(st), C.c_void_p(stream_ptr)))
        return st.as_dict()

    DBG = {"big_dense": 0, "big_sparse": 1, "neq_tiles": 2, "neq_overlap": 3, "small_nodes": 4, "neq_lean": 8, "neq_lean_passes": 9, "neq_lean_handover": 10}

    def debug_counters(self, stream_ptr: int = 0) -> dict:
        """Kernel-internal diagnostic counters since the last stats_reset (pcp_debug_counters, ABI v6): which code paths ran."""
        out = (C.c_uint64 * 16)()
        self._check(self._L.pcp_debug_counters(self._h, out, 16, C.c_void_p(stream_ptr)))
        d = {k: int(out[i]) for k, i in self.DBG.items()}
        d["raw"] = [int(x) for x in out]
        return d

    def last_plan(self) -> dict:
        """pcp_last_plan: the launch geometry of the last propagate call."""
        pl = PcpPlan()
        self._check(self._L.pcp_last_plan(self._h, C.byref(pl)))
        return pl.as_dict()

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        self._check(self._L.pcp_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)


STEAL_MODES = ("host", "device")


def _check_steal(who, steal, dist=None):
    """``steal`` of the Interval forest drivers: "host" or "device"; "device" runs on one rank."""
    if steal not in STEAL_MODES:
        raise ValueError(f"{who}: steal must be 'host' or 'device', not {steal!r}")
    if steal == "device" and dist is not None and dist.get_world_size() > 1:
        raise ValueError(f"{who}: steal='device' runs on one rank (the refill across ranks works from the host's copy of sp)")


def _check_brancher(brancher, val):
    if brancher not in ("split", "enumerate"):
        raise ValueError(f"brancher must be 'split' or 'enumerate', not {brancher!r}")
    if brancher == "enumerate" and val not in VAL_MODES:
        raise ValueError(f"val must be 'middle' or 'min', not {val!r}")


def _check_forest_brancher(who, brancher, val, small, dist, root_excl=None) -> bool:
    """The distributor of an Interval forest: True under Enumerate.  Through ``small=True`` Enumerate runs in the small-store forest, on one
    rank; Context.dfs_forest_enum / search_forest.forest_enumerate choose the forest by the store and reach the formula-store forest too."""
    _check_brancher(brancher, val)
    enum = brancher == "enumerate"
    if enum and not small:
        raise ValueError(f"{who}: brancher='enumerate' needs small=True here (the small-store forest) — Context.dfs_forest_enum / search_forest.forest_enumerate run Enumerate over every Interval store: the formula-store forest and the all-XNeqY in-kernel forest included")
    if enum and dist is not None:
        raise ValueError(f"{who}: brancher='enumerate' does not run on several ranks (moving exclusion lists between ranks is not built)")
    if root_excl is not None and not enum:
        raise ValueError(f"{who}: root_excl needs brancher='enumerate'")
    return enum


def _check_collect_set(who, collect_solutions, sink_capacity, bnb=False):
    """collect_solutions of a set-mode forest: both write into a set solution sink; branch and bound does not."""
    if not collect_solutions:
        return
    if bnb:
        raise ValueError(f"{who}: collect_solutions does not go with branch and bound (it keeps best_solution; the entries refuse a set solution sink)")
    if int(sink_capacity) < 1:
        raise ValueError(f"{who}: sink_capacity must be at least 1, not {sink_capacity}")


def _check_collect(who, collect_solutions, sink_capacity, small, formulas, dist, bnb=False):
    """collect_solutions of an Interval forest: the formula-store and the small-store forest write into a solution sink, on one rank."""
    if not collect_solutions:
        return
    if bnb:
        raise ValueError(f"{who}: collect_solutions does not go with branch and bound (it keeps best_solution; the entries refuse a solution sink)")
    if not small and not formulas:
        raise ValueError(f"{who}: collect_solutions needs formulas=True or small=True (the all-XNeqY entry behind it refuses the context's solution sink — Context.dfs_forest_neq_solutions / search_forest.forest_solutions return that forest's solutions; small=True takes an all-XNeqY store within its limits)")
    if dist is not None:
        raise ValueError(f"{who}: collect_solutions does not run on several ranks (gathering the sinks is not built)")
    if int(sink_capacity) < 1:
        raise ValueError(f"{who}: sink_capacity must be at least 1, not {sink_capacity}")


def full_active(n_nodes: int, n_units: int) -> np.ndarray:
    """`active` rows with every unit set (Store::alloc inserts each new propagator, propagation/store.rs:227)."""
    words = (n_units + 63) // 64
    a = np.full((n_nodes, words), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    if words and n_units % 64:
        a[:, -1] = np.uint64((1 << (n_units % 64)) - 1)
    return a
