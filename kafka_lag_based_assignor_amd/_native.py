"""ctypes binding of the C ABI in include/lagassign.h (liblagassign.so).

This is the same boundary a JNI shim binds.  There is no fallback: if
the shared object is missing or no gfx950 device is usable, calls raise.
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LA_LIB_PATH") or os.path.join(_HERE, "liblagassign.so")   # LA_LIB_PATH: A/B runs of two builds

LA_OK = 0
LA_EINVAL, LA_ENOMEM, LA_EHIP, LA_ENODEV, LA_ESHAPE = -1, -2, -3, -4, -5
LA_RESET_LATEST, LA_RESET_EARLIEST = 0, 1
LA_ALGO_AUTO, LA_ALGO_ROUNDS, LA_ALGO_ARGMIN, LA_ALGO_ROUNDS_WIDE = 0, 1, 2, 3
LA_FLAG_INDEX64, LA_FLAG_DEFER_WIDE, LA_FLAG_RAGGED, LA_FLAG_SHAPE_CLASSES = 1, 2, 4, 8
LA_FLAG_PROFILE, LA_FLAG_NO_SAMPLE_SORT, LA_FLAG_SAMPLE_TIGHT = 16, 32, 64
LA_FLAG_SORT_MULTIKERNEL = 128
LA_FLAG_NO_RUN_MERGE = 256
LA_FLAG_NO_MOVED_SORT = 2048
LA_FLAG_SERIAL_LARGE = 512
LA_FLAG_BOUNDS = 1024
LA_FLAG_WIRE_OUT = 4096
LA_FLAG_VERIFY_LARGE = 8192
LA_FEATURE_ATOMIC_RANK = 1
LA_PIPELINE_ONE_COPY, LA_PIPELINE_LANES, LA_PIPELINE_STREAMS, LA_PIPELINE_ZERO_COPY, LA_PIPELINE_MAPPED = 0, 1, 2, 3, 4
LA_CREATE_LANES_MASK, LA_CREATE_SPLIT_ALWAYS = 0xF, 0x10
LA_HINT_BOUNDS = 1
# la_member_loads_device: up to this many members the bins of the roll-up live in LDS, beyond it every element is one global
# atomic add (kLoadsLdsMaxMembers of csrc/la_kernels.h; results are the same, tests run both sides)
LOADS_LDS_MAX_MEMBERS = 4095
# la_assignment_moves_device: topics up to MOVES_LDS_MAX_PARTITIONS are joined in one workgroup's LDS (larger ones through a table
# in device memory, found from h_part_off); up to MOVES_LDS_MAX_MEMBERS the gained / lost counts are LDS bins (kMovesLdsMaxPartitions /
# kMovesLdsMaxMembers of csrc/la_kernels.h; results are the same, tests run both sides)
MOVES_LDS_MAX_PARTITIONS = 4096
MOVES_LDS_MAX_MEMBERS = 4096
# la_assignment_moves_device with two layouts: d_prev_owner of a partition that has no previous entry (it was added)
LA_MOVES_NO_PREVIOUS = -2
# la_verify_assignment_device: d_topic_verdict[t] is 0 (certified) or a mask of these; a topic of more than VERIFY_MAX_PARTITIONS
# partitions or VERIFY_MAX_CONSUMERS consumers reads LA_VERDICT_UNCHECKED (kVerifyMax* of csrc/la_kernels.h) unless the batch carries
# LA_FLAG_VERIFY_LARGE: such topics then go through tables in device memory, up to VERIFY_GLOBAL_MAX_PARTITIONS partitions and any
# consumer count, in at most VERIFY_MAX_LAUNCHES kernel launches per call (kVerifyGlobalMaxPartitions / kVerifyMaxLaunches)
LA_VERDICT_IDS, LA_VERDICT_ORDER, LA_VERDICT_OWNER, LA_VERDICT_GREEDY, LA_VERDICT_TOTALS, LA_VERDICT_UNCHECKED = 1, 2, 4, 8, 16, 32
VERIFY_MAX_PARTITIONS = 4096
VERIFY_MAX_CONSUMERS = 4096
VERIFY_GLOBAL_MAX_PARTITIONS = (1 << 30) - 2
VERIFY_MAX_LAUNCHES = 7
# la_cooperative_adjust_device: insert the owned entries, look the target up (kCoopLaunches of csrc/la_coop.h); its per-member
# counts are LDS bins up to MOVES_LDS_MAX_MEMBERS members, as the moves call's
COOP_MAX_LAUNCHES = 2
# la_cooperative_round[_device]: a call within ALL four limits (entries N, owned entries, members M, topics T) is one launch of one
# workgroup; any other, or one with LA_COOP_FORCE_TABLE, the table form plus the grouping (kCoopSmall* of csrc/la_coop.h; results
# are the same, tests run both sides)
COOP_SMALL_ENTRIES = 2048
COOP_SMALL_OWNED = 2048
COOP_SMALL_MEMBERS = 2046
COOP_SMALL_TOPICS = 2048
LA_COOP_FORCE_TABLE = 1
# la_cooperative_round_sticky_device: within ALL four limits, and without LA_COOP_FORCE_TABLE, one launch of one workgroup;
# any other call is the chain of the three calls it replaces (LA_COOP_STICKY_* of lagassign.h, kCoopSticky* of csrc/la_coop.h)
LA_COOP_STICKY_ENTRIES = COOP_STICKY_ENTRIES = 2048
LA_COOP_STICKY_OWNED = COOP_STICKY_OWNED = 2048
LA_COOP_STICKY_MEMBERS = COOP_STICKY_MEMBERS = 2046
LA_COOP_STICKY_TOPICS = COOP_STICKY_TOPICS = 2048
# la_sticky_ties_device / la_cooperative_round_sticky_device with LA_FLAG_STICKY_LARGE in the batch's flags (h_part_off then
# required), la_assign_batch_cooperative_sticky with LA_COOP_STICKY_LARGE in coop.flags: topics of more than VERIFY_MAX_PARTITIONS
# and up to STICKY_GLOBAL_MAX_PARTITIONS partitions are re-matched through tables in device memory instead of being passed
# through, in at most STICKY_GLOBAL_LAUNCHES more kernel launches per call whatever their number and size (kStickyGlobalLaunches /
# kStickyGlobalMaxPartitions of csrc/la_kernels.h; 19 while the call's large topics hold fewer than 2^29 partitions together)
LA_FLAG_STICKY_LARGE = 16384
LA_COOP_STICKY_LARGE = 2
STICKY_GLOBAL_LAUNCHES = 43
STICKY_GLOBAL_MAX_PARTITIONS = (1 << 30) - 2
# la_assign_pinned_device: one workgroup holds a topic in its LDS, up to these sizes (kPinnedMax* of csrc/la_coop.h); a larger
# topic is LA_ESHAPE -- from sync() for the device call, at the call for assign_batch_cooperative(pinned=True).  At most
# PINNED_MAX_LAUNCHES kernels: insert the owned entries, do the topics
LA_PINNED_MAX_PARTITIONS = PINNED_MAX_PARTITIONS = 4096
LA_PINNED_MAX_CONSUMERS = PINNED_MAX_CONSUMERS = 2048
PINNED_MAX_LAUNCHES = 2
LA_COOP_PINNED = 4
# LA_FLAG_PINNED_LARGE in the batch's flags (h_part_off / h_cons_off then required): topics of more than PINNED_MAX_PARTITIONS and
# up to PINNED_LARGE_MAX_PARTITIONS partitions go through the large form (csrc/la_pinned_large.hip) in at most
# PINNED_LARGE_LAUNCHES more kernels; LA_COOP_PINNED_LARGE is the same for assign_batch_cooperative(pinned=True, pinned_large=True)
LA_FLAG_PINNED_LARGE = 32768
LA_COOP_PINNED_LARGE = 8
LA_PINNED_LARGE_MAX_PARTITIONS = PINNED_LARGE_MAX_PARTITIONS = (1 << 30) - 2
LA_PINNED_LARGE_LAUNCHES = PINNED_LARGE_LAUNCHES = 42

EXPORTED_SYMBOLS = (
    "la_create", "la_destroy", "la_last_error", "la_version", "la_compute_lag",
    "la_assign_batch", "la_assign_batch_lags", "la_assign_batch_device", "la_sync", "la_stream",
    "la_group_by_member", "la_group_by_member_device", "la_group_last_by_member",
    "la_device_count", "la_create_multi", "la_shard_count", "la_shard_device", "la_plan_shards",
    "la_last_shard_bounds", "la_host_alloc", "la_host_free", "la_last_phase_times", "la_device_features",
    "la_shard_stream", "la_assign_batch_device_on", "la_sync_on", "la_group_by_member_device_on", "la_last_pipeline",
    "la_allgather_results", "la_assign_batch_grouped",
    "la_wire_format_for", "la_pack_results_on", "la_unpack_results_on", "la_allgather_packed",
    "la_assign_batch_sparse", "la_assign_batch_grouped_sparse",
    "la_hint_next_call", "la_last_launches", "la_last_phase_times_sized", "la_wake",
    "la_member_loads_device", "la_member_loads_device_on",
    "la_assignment_moves_device", "la_assignment_moves_device_on",
    "la_verify_assignment_device", "la_verify_assignment_device_on",
    "la_cooperative_adjust_device",
    "la_cooperative_round_device", "la_cooperative_round",
    "la_assign_batch_cooperative",
    "la_sticky_ties_device",
    "la_cooperative_round_sticky_device", "la_assign_batch_cooperative_sticky",
    "la_assign_pinned_device",
)

_i64p = ctypes.POINTER(ctypes.c_int64)
_i32p = ctypes.POINTER(ctypes.c_int32)
_vp = ctypes.c_void_p      # what the array parameters are declared as: an address (int), None, or any ctypes pointer
_byte = ctypes.c_char


class LagAssignError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__("liblagassign error %d: %s" % (code, message))
        self.code = code


class DeviceBatch(ctypes.Structure):
    """struct la_device_batch"""
    _fields_ = [
        ("n_topics", ctypes.c_int32), ("reset_mode", ctypes.c_int32),
        ("algo", ctypes.c_int32), ("flags", ctypes.c_int32),
        ("n_partitions", ctypes.c_int64), ("n_consumers", ctypes.c_int64),
        ("max_partitions_per_topic", ctypes.c_int64), ("max_consumers_per_topic", ctypes.c_int64),
        ("d_part_off", ctypes.c_void_p), ("d_partition_id", ctypes.c_void_p),
        ("d_begin_off", ctypes.c_void_p), ("d_end_off", ctypes.c_void_p),
        ("d_committed_off", ctypes.c_void_p), ("d_lag", ctypes.c_void_p),
        ("d_cons_off", ctypes.c_void_p), ("d_cons_rank", ctypes.c_void_p),
        ("d_out_partition", ctypes.c_void_p), ("d_out_member_rank", ctypes.c_void_p),
        ("d_out_total_lag", ctypes.c_void_p),
        ("h_part_off", _i64p), ("h_cons_off", _i64p),
        ("max_lag_hint", ctypes.c_int64), ("max_partition_id_hint", ctypes.c_int64),
        ("d_out_wire", ctypes.c_void_p), ("wire_elem_bytes", ctypes.c_int32), ("wire_id_bits", ctypes.c_int32),
    ]


class CallHints(ctypes.Structure):
    """struct la_call_hints"""
    _fields_ = [("struct_size", ctypes.c_int32), ("flags", ctypes.c_int32), ("max_lag", ctypes.c_int64),
                ("max_partition_id", ctypes.c_int64)]


class WireFormat(ctypes.Structure):
    """struct la_wire_format: one element = ((member rank + 1) << id_bits) | partition id, in elem_bytes bytes"""
    _fields_ = [("elem_bytes", ctypes.c_int32), ("id_bits", ctypes.c_int32)]

    @property
    def dtype(self):
        return {2: np.uint16, 4: np.uint32, 8: np.uint64}[int(self.elem_bytes)]


class MovesArgs(ctypes.Structure):
    """struct la_moves_args (device addresses as ints, None / 0 = NULL; struct_size is filled in by assignment_moves_device)"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("n_topics", ctypes.c_int32),
        ("n_partitions", ctypes.c_int64), ("max_partitions_per_topic", ctypes.c_int64),
        ("d_part_off", ctypes.c_void_p), ("h_part_off", _i64p),
        ("d_out_partition", ctypes.c_void_p), ("d_out_member_rank", ctypes.c_void_p),
        ("d_prev_partition", ctypes.c_void_p), ("d_prev_member_rank", ctypes.c_void_p),
        ("n_members", ctypes.c_int32), ("n_prev_members", ctypes.c_int32),
        ("d_prev_rank_map", ctypes.c_void_p),
        ("d_prev_owner", ctypes.c_void_p), ("d_topic_moved", ctypes.c_void_p),
        ("d_member_gained", ctypes.c_void_p), ("d_member_lost", ctypes.c_void_p), ("d_moved", ctypes.c_void_p),
        # two layouts (d_prev_part_off set); left at 0 / NULL the call is the one-layout form
        ("n_prev_topics", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_prev_partitions", ctypes.c_int64),
        ("d_prev_part_off", ctypes.c_void_p), ("h_prev_part_off", _i64p),
        ("d_prev_topic", ctypes.c_void_p), ("h_prev_topic", ctypes.POINTER(ctypes.c_int32)),
        ("d_topic_added", ctypes.c_void_p), ("d_topic_removed", ctypes.c_void_p),
        ("d_added", ctypes.c_void_p), ("d_removed", ctypes.c_void_p),
    ]


class CoopArgs(ctypes.Structure):
    """struct la_coop_args (device addresses as ints, None / 0 = NULL; struct_size is filled in by cooperative_adjust_device)"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("n_topics", ctypes.c_int32), ("n_partitions", ctypes.c_int64),
        ("d_part_off", ctypes.c_void_p), ("d_out_partition", ctypes.c_void_p), ("d_out_member_rank", ctypes.c_void_p),
        ("n_members", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_owned", ctypes.c_int64),
        ("d_owned_member_off", ctypes.c_void_p), ("d_owned_topic", ctypes.c_void_p), ("d_owned_partition", ctypes.c_void_p),
        ("d_prev_owner", ctypes.c_void_p), ("d_coop_member_rank", ctypes.c_void_p),
        ("d_member_kept", ctypes.c_void_p), ("d_member_fresh", ctypes.c_void_p), ("d_member_pending", ctypes.c_void_p),
        ("d_member_release", ctypes.c_void_p), ("d_topic_withheld", ctypes.c_void_p), ("d_summary", ctypes.c_void_p),
    ]


class StickyArgs(ctypes.Structure):
    """struct la_sticky_args (device addresses as ints, None / 0 = NULL; struct_size is filled in by sticky_ties_device)"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("d_prev_owner", ctypes.c_void_p), ("d_sticky_partition", ctypes.c_void_p),
        ("d_topic_kept", ctypes.c_void_p), ("d_topic_saved", ctypes.c_void_p), ("d_summary", ctypes.c_void_p),
    ]


class CoopRoundArgs(ctypes.Structure):
    """struct la_coop_round_args (addresses as ints, None / 0 = NULL; struct_size is filled in by cooperative_round_device).
    `adjust` is the CoopArgs of cooperative_adjust_device; for la_cooperative_round every address is host memory."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("flags", ctypes.c_int32), ("adjust", CoopArgs),
        ("member_off", ctypes.c_void_p), ("grouped_topic", ctypes.c_void_p), ("grouped_partition", ctypes.c_void_p),
    ]


class CoopStickyArgs(ctypes.Structure):
    """struct la_coop_sticky_args (device addresses as ints, None / 0 = NULL; struct_size is filled in by
    cooperative_round_sticky_device).  `round` is the CoopRoundArgs of cooperative_round_device; its target fields (n_topics,
    n_partitions, d_part_off, d_out_partition, d_out_member_rank) are not looked at: the target is the batch's."""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("flags", ctypes.c_int32), ("round", CoopRoundArgs),
        ("d_sticky_partition", ctypes.c_void_p), ("d_topic_kept", ctypes.c_void_p), ("d_topic_saved", ctypes.c_void_p),
        ("d_sticky_summary", ctypes.c_void_p),
    ]


class PinnedArgs(ctypes.Structure):
    """struct la_pinned_args (device addresses as ints, None / 0 = NULL; struct_size is filled in by assign_pinned_device)"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_members", ctypes.c_int32), ("reserved2", ctypes.c_int32),
        ("n_owned", ctypes.c_int64),
        ("d_owned_member_off", ctypes.c_void_p), ("d_owned_topic", ctypes.c_void_p), ("d_owned_partition", ctypes.c_void_p),
        ("d_topic_free", ctypes.c_void_p), ("d_summary", ctypes.c_void_p),
    ]


class CoopRound(NamedTuple):
    """What Context.cooperative_round returns: the eight outputs of the adjusted assignment, then every member's list of it."""
    prev_owner: np.ndarray
    coop_member_rank: np.ndarray
    kept: np.ndarray
    fresh: np.ndarray
    pending: np.ndarray
    release: np.ndarray
    topic_withheld: np.ndarray
    summary: np.ndarray
    member_off: np.ndarray
    grouped_topic: np.ndarray
    grouped_partition: np.ndarray


class AssignCoopArgs(ctypes.Structure):
    """struct la_assign_coop_args (host addresses as ints, None / 0 = NULL)"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("flags", ctypes.c_int32), ("n_topics", ctypes.c_int32), ("reset_mode", ctypes.c_int32),
        ("part_off", ctypes.c_void_p), ("partition_id", ctypes.c_void_p), ("lag", ctypes.c_void_p),
        ("begin_off", ctypes.c_void_p), ("end_off", ctypes.c_void_p), ("committed_off", ctypes.c_void_p),
        ("n_none", ctypes.c_int64), ("none_index", ctypes.c_void_p), ("none_begin", ctypes.c_void_p),
        ("cons_off", ctypes.c_void_p), ("cons_rank", ctypes.c_void_p),
        ("n_members", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("n_owned", ctypes.c_int64), ("owned_member_off", ctypes.c_void_p), ("owned_topic", ctypes.c_void_p),
        ("owned_partition", ctypes.c_void_p),
        ("member_off", ctypes.c_void_p), ("grouped_topic", ctypes.c_void_p), ("grouped_partition", ctypes.c_void_p),
        ("out_total_lag", ctypes.c_void_p), ("out_partition", ctypes.c_void_p), ("out_member_rank", ctypes.c_void_p),
        ("prev_owner", ctypes.c_void_p), ("coop_member_rank", ctypes.c_void_p),
        ("member_kept", ctypes.c_void_p), ("member_fresh", ctypes.c_void_p), ("member_pending", ctypes.c_void_p),
        ("member_release", ctypes.c_void_p), ("topic_withheld", ctypes.c_void_p), ("summary", ctypes.c_void_p),
    ]


class AssignCoop(NamedTuple):
    """What Context.assign_batch_cooperative returns (and takes as `out`): the TARGET (what the assign call returns) and its
    totals, the eight outputs of the adjusted assignment, then every member's list of it.  A None entry was not asked for."""
    out_partition: Optional[np.ndarray]
    out_member_rank: Optional[np.ndarray]
    totals: Optional[np.ndarray]
    prev_owner: Optional[np.ndarray]
    coop_member_rank: Optional[np.ndarray]
    kept: Optional[np.ndarray]
    fresh: Optional[np.ndarray]
    pending: Optional[np.ndarray]
    release: Optional[np.ndarray]
    topic_withheld: Optional[np.ndarray]
    summary: Optional[np.ndarray]
    member_off: np.ndarray
    grouped_topic: Optional[np.ndarray]
    grouped_partition: np.ndarray


class AssignStickyArgs(ctypes.Structure):
    """struct la_assign_sticky_args (host addresses as ints, None / 0 = NULL)"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("coop", AssignCoopArgs),
        ("sticky_partition", ctypes.c_void_p), ("topic_kept", ctypes.c_void_p), ("topic_saved", ctypes.c_void_p),
        ("sticky_summary", ctypes.c_void_p),
    ]


class AssignSticky(NamedTuple):
    """What Context.assign_batch_cooperative_sticky returns: `coop`, an AssignCoop whose target entries (out_partition,
    out_member_rank, totals) describe the TARGET and whose other entries describe the STICKY order, and the four sticky outputs."""
    coop: AssignCoop
    sticky_partition: np.ndarray
    topic_kept: np.ndarray
    topic_saved: np.ndarray
    sticky_summary: np.ndarray


class PhaseTimes(ctypes.Structure):
    """struct la_phase_times"""
    _fields_ = [("n_partitions", ctypes.c_int64), ("id_passes", ctypes.c_int32), ("key_passes", ctypes.c_int32),
                ("keys_ms", ctypes.c_float), ("sort_ms", ctypes.c_float), ("greedy_ms", ctypes.c_float),
                ("keys_first", ctypes.c_int32), ("redone", ctypes.c_int32)]


_lib: Optional[ctypes.CDLL] = None


def load() -> ctypes.CDLL:
    """Loads liblagassign.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -m kafka_lag_based_assignor_amd.build` "
            "(needs hipcc). There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch bundles its own libamdhip64.so.7.  Importing torch
    # first makes liblagassign's NEEDED libamdhip64.so.7 resolve to that already-loaded copy,
    # so torch tensors, torch streams and our kernels share one runtime.  (Two runtimes in one
    # process fail at device discovery.)  Without torch -- e.g. under a JVM -- the system
    # ROCm runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    L.la_version.restype = ctypes.c_int
    L.la_create.restype = ctypes.c_int
    L.la_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_uint]
    L.la_create_multi.restype = ctypes.c_int
    L.la_create_multi.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                  ctypes.c_uint]
    L.la_device_count.restype = ctypes.c_int
    L.la_device_count.argtypes = []
    L.la_shard_count.restype = ctypes.c_int
    L.la_shard_count.argtypes = [ctypes.c_void_p]
    L.la_shard_device.restype = ctypes.c_int
    L.la_shard_device.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.la_device_features.restype = ctypes.c_int
    L.la_device_features.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.la_plan_shards.restype = ctypes.c_int
    L.la_plan_shards.argtypes = [ctypes.c_int32, _vp, ctypes.c_int32, _vp]
    L.la_last_shard_bounds.restype = ctypes.c_int
    L.la_last_shard_bounds.argtypes = [ctypes.c_void_p, _vp, ctypes.c_int32]
    L.la_host_alloc.restype = ctypes.c_void_p
    L.la_host_alloc.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    L.la_host_free.restype = None
    L.la_host_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.la_destroy.restype = None
    L.la_destroy.argtypes = [ctypes.c_void_p]
    L.la_last_error.restype = ctypes.c_char_p
    L.la_last_error.argtypes = [ctypes.c_void_p]
    L.la_compute_lag.restype = ctypes.c_int
    L.la_compute_lag.argtypes = [ctypes.c_void_p, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int32, _vp]
    L.la_assign_batch.restype = ctypes.c_int
    L.la_assign_batch.argtypes = [ctypes.c_void_p, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp,
                                  ctypes.c_int32, _vp, _vp, _vp, _vp, _vp]
    L.la_assign_batch_lags.restype = ctypes.c_int
    L.la_assign_batch_grouped.argtypes = [ctypes.c_void_p, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp,
                                          ctypes.c_int32, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp]
    L.la_assign_batch_grouped.restype = ctypes.c_int
    L.la_assign_batch_lags.argtypes = [ctypes.c_void_p, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp]
    L.la_assign_batch_device.restype = ctypes.c_int
    L.la_assign_batch_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(DeviceBatch), ctypes.c_void_p]
    L.la_sync.restype = ctypes.c_int
    L.la_sync.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.la_last_phase_times.restype = ctypes.c_int
    L.la_last_phase_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(PhaseTimes)]
    L.la_stream.restype = ctypes.c_void_p
    L.la_stream.argtypes = [ctypes.c_void_p]
    L.la_group_by_member.restype = ctypes.c_int
    L.la_group_by_member.argtypes = [ctypes.c_void_p, ctypes.c_int32, _vp, _vp, _vp, ctypes.c_int32,
                                     _vp, _vp, _vp]
    L.la_group_last_by_member.restype = ctypes.c_int
    L.la_group_last_by_member.argtypes = [ctypes.c_void_p, ctypes.c_int32, _vp, _vp, _vp]
    L.la_group_by_member_device.restype = ctypes.c_int
    L.la_group_by_member_device.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.la_allgather_results.restype = ctypes.c_int
    L.la_allgather_results.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_void_p),
                                       ctypes.POINTER(ctypes.c_void_p)]
    L.la_last_pipeline.restype = ctypes.c_int
    L.la_last_pipeline.argtypes = [ctypes.c_void_p]
    L.la_wire_format_for.restype = ctypes.c_int
    L.la_wire_format_for.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(WireFormat)]
    L.la_pack_results_on.restype = ctypes.c_int
    L.la_pack_results_on.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(WireFormat), ctypes.c_void_p, ctypes.c_void_p]
    L.la_unpack_results_on.restype = ctypes.c_int
    L.la_unpack_results_on.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                       ctypes.POINTER(WireFormat), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.la_allgather_packed.restype = ctypes.c_int
    L.la_allgather_packed.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(ctypes.c_void_p)]
    L.la_assign_batch_sparse.restype = ctypes.c_int
    L.la_assign_batch_sparse.argtypes = [ctypes.c_void_p, ctypes.c_int32, _vp, _vp, _vp, _vp, ctypes.c_int32,
                                         ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    L.la_assign_batch_grouped_sparse.restype = ctypes.c_int
    L.la_assign_batch_grouped_sparse.argtypes = [ctypes.c_void_p, ctypes.c_int32, _vp, _vp, _vp, _vp, ctypes.c_int32,
                                                 ctypes.c_int64, _vp, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp,
                                                 _vp, _vp]
    L.la_shard_stream.restype = ctypes.c_void_p
    L.la_shard_stream.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.la_assign_batch_device_on.restype = ctypes.c_int
    L.la_assign_batch_device_on.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.la_sync_on.restype = ctypes.c_int
    L.la_sync_on.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    L.la_group_by_member_device_on.restype = ctypes.c_int
    L.la_group_by_member_device_on.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_int64,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.la_hint_next_call.restype = ctypes.c_int
    L.la_hint_next_call.argtypes = [ctypes.c_void_p, ctypes.POINTER(CallHints)]
    L.la_last_launches.restype = ctypes.c_int64
    L.la_last_launches.argtypes = [ctypes.c_void_p]
    L.la_wake.restype = ctypes.c_int
    L.la_wake.argtypes = [ctypes.c_void_p]
    L.la_last_phase_times_sized.restype = ctypes.c_int
    L.la_last_phase_times_sized.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    # added without an ABI bump: found by symbol lookup (an older library simply lacks them)
    if hasattr(L, "la_member_loads_device_on"):
        _loads = [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.la_member_loads_device.restype = ctypes.c_int
        L.la_member_loads_device.argtypes = [ctypes.c_void_p] + _loads
        L.la_member_loads_device_on.restype = ctypes.c_int
        L.la_member_loads_device_on.argtypes = [ctypes.c_void_p, ctypes.c_int] + _loads
    if hasattr(L, "la_assignment_moves_device_on"):
        L.la_assignment_moves_device.restype = ctypes.c_int
        L.la_assignment_moves_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(MovesArgs), ctypes.c_void_p]
        L.la_assignment_moves_device_on.restype = ctypes.c_int
        L.la_assignment_moves_device_on.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(MovesArgs), ctypes.c_void_p]
    if hasattr(L, "la_verify_assignment_device_on"):
        L.la_verify_assignment_device.restype = ctypes.c_int
        L.la_verify_assignment_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(DeviceBatch), ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p]
        L.la_verify_assignment_device_on.restype = ctypes.c_int
        L.la_verify_assignment_device_on.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(DeviceBatch), ctypes.c_void_p,
                                                     ctypes.c_void_p, ctypes.c_void_p]
    if hasattr(L, "la_cooperative_adjust_device"):
        L.la_cooperative_adjust_device.restype = ctypes.c_int
        L.la_cooperative_adjust_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(CoopArgs), ctypes.c_void_p]
    if hasattr(L, "la_cooperative_round_device"):
        L.la_cooperative_round_device.restype = ctypes.c_int
        L.la_cooperative_round_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(CoopRoundArgs), ctypes.c_void_p]
        L.la_cooperative_round.restype = ctypes.c_int
        L.la_cooperative_round.argtypes = [ctypes.c_void_p, ctypes.POINTER(CoopRoundArgs)]
    if hasattr(L, "la_assign_batch_cooperative"):
        L.la_assign_batch_cooperative.restype = ctypes.c_int
        L.la_assign_batch_cooperative.argtypes = [ctypes.c_void_p, ctypes.POINTER(AssignCoopArgs)]
    if hasattr(L, "la_sticky_ties_device"):
        L.la_sticky_ties_device.restype = ctypes.c_int
        L.la_sticky_ties_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(DeviceBatch), ctypes.POINTER(StickyArgs), ctypes.c_void_p]
    if hasattr(L, "la_cooperative_round_sticky_device"):
        L.la_cooperative_round_sticky_device.restype = ctypes.c_int
        L.la_cooperative_round_sticky_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(DeviceBatch), ctypes.POINTER(CoopStickyArgs),
                                                         ctypes.c_void_p]
    if hasattr(L, "la_assign_batch_cooperative_sticky"):
        L.la_assign_batch_cooperative_sticky.restype = ctypes.c_int
        L.la_assign_batch_cooperative_sticky.argtypes = [ctypes.c_void_p, ctypes.POINTER(AssignStickyArgs)]
    if hasattr(L, "la_sticky_ties_device_on"):
        L.la_sticky_ties_device_on.restype = ctypes.c_int
        L.la_sticky_ties_device_on.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(DeviceBatch), ctypes.POINTER(StickyArgs),
                                               ctypes.c_void_p]
    if hasattr(L, "la_assign_pinned_device"):
        L.la_assign_pinned_device.restype = ctypes.c_int
        L.la_assign_pinned_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(DeviceBatch), ctypes.POINTER(PinnedArgs), ctypes.c_void_p]
    _lib = L
    return L


def _a64(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.int64)


def _a32(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.int32)


def _addr(a: Optional[np.ndarray]):
    """Address of a contiguous array's first element for a c_void_p parameter.  A small rebalance is a dozen pointers per call
    and `a.ctypes.data_as(...)` costs 1-2.5 us apiece (it builds a helper object and a typed pointer); the buffer protocol gives
    the same address in 0.3 us.  The CALLER keeps `a` alive across the call (the wrappers below hold every array in a local).
    Read-only and empty arrays do not export a writable buffer: they take the slow way."""
    if a is None:
        return None
    try:
        return ctypes.addressof(_byte.from_buffer(a))
    except (TypeError, ValueError, BufferError):
        return a.ctypes.data


_p64 = _addr       # (dtype and contiguity are the business of _a64 / _a32 before)
_p32 = _addr


def _check_out3(out, n: int, k: int):
    """Caller-owned result buffers (out_partition int32[N], out_member_rank int32[N], totals int64[K] or None): the library writes
    N / K contiguous elements at each address, so anything else -- a strided view above all -- is refused here."""
    out_p, out_m, out_t = out
    ok = (isinstance(out_p, np.ndarray) and isinstance(out_m, np.ndarray) and out_p.dtype == np.int32 and out_m.dtype == np.int32 and
          out_p.size == n and out_m.size == n and out_p.flags.c_contiguous and out_m.flags.c_contiguous and
          (out_t is None or (isinstance(out_t, np.ndarray) and out_t.dtype == np.int64 and out_t.size == k and out_t.flags.c_contiguous)))
    if not ok:
        raise ValueError("out buffers must be contiguous int32[N], int32[N], int64[K]")
    return out_p, out_m, out_t


def _check_out_grouped(out, m: int, n: int, k: int):
    """Caller-owned grouped result buffers (member_off int64[M+1], grouped_topic int32[N] or None, grouped_partition int32[N],
    totals int64[K] or None): contiguous, of the right type and size, as for _check_out3."""
    off, g_t, g_p, out_t = out

    def ok(a, dtype, size, optional=False):
        if a is None:
            return optional
        return isinstance(a, np.ndarray) and a.dtype == dtype and a.size == size and a.flags.c_contiguous

    if not (ok(off, np.int64, m + 1) and ok(g_t, np.int32, n, True) and ok(g_p, np.int32, n) and ok(out_t, np.int64, k, True)):
        raise ValueError("out buffers must be contiguous int64[M+1], int32[N] or None, int32[N], int64[K] or None")
    return off, g_t, g_p, out_t


def _check_out_coop(out: AssignCoop, m: int, n: int, k: int, t: int) -> AssignCoop:
    """Caller-owned buffers of assign_batch_cooperative: contiguous, of the right type and size, as for _check_out_grouped.
    member_off and grouped_partition are required, the target's two arrays come together, every other entry may be None."""
    def ok(a, dtype, size, optional=True):
        if a is None:
            return optional
        return isinstance(a, np.ndarray) and a.dtype == dtype and a.size == size and a.flags.c_contiguous

    if not (isinstance(out, AssignCoop) and (out.out_partition is None) == (out.out_member_rank is None) and
            ok(out.out_partition, np.int32, n) and ok(out.out_member_rank, np.int32, n) and ok(out.totals, np.int64, k) and
            ok(out.prev_owner, np.int32, n) and ok(out.coop_member_rank, np.int32, n) and ok(out.kept, np.int64, m) and
            ok(out.fresh, np.int64, m) and ok(out.pending, np.int64, m) and ok(out.release, np.int64, m) and
            ok(out.topic_withheld, np.int64, t) and ok(out.summary, np.int64, 6) and ok(out.member_off, np.int64, m + 1, False) and
            ok(out.grouped_topic, np.int32, n) and ok(out.grouped_partition, np.int32, n, False)):
        raise ValueError("out must be an AssignCoop of contiguous arrays: int32[N] x2 (both or neither), int64[K], int32[N] x2, "
                         "int64[M] x4, int64[T], int64[6], int64[M+1] (required), int32[N], int32[N] (required); None = not wanted")
    return out


def plan_shards(part_off, n_shards: int) -> np.ndarray:
    """la_plan_shards: the library's own planner (pure host code, no device needed).  Returns int32
    bounds[n_shards + 1]: shard r owns topics [bounds[r], bounds[r+1])."""
    part_off = _a64(part_off)
    bounds = np.zeros(n_shards + 1, dtype=np.int32)
    rc = load().la_plan_shards(part_off.size - 1, _p64(part_off), n_shards, _p32(bounds))
    if rc != LA_OK:
        raise LagAssignError(rc, "la_plan_shards: bad arguments")
    return bounds


def wire_format_for(max_partition_id: int, n_members: int) -> WireFormat:
    """la_wire_format_for (pure host code): the narrowest wire element for ids in [0, max_partition_id] (negative: any
    int32) and member ranks in [-1, n_members)."""
    f = WireFormat()
    rc = load().la_wire_format_for(int(max_partition_id), int(n_members), ctypes.byref(f))
    if rc != LA_OK:
        raise LagAssignError(rc, "la_wire_format_for")
    return f


def sparse_begin(begin, committed):
    """(none_index int64[m], none_begin int64[m]) of a dense `begin` array: the positions without a committed offset, ascending
    -- what a marshaller that knows `md == null` hands to la_assign_batch_sparse instead of the dense array."""
    idx = np.flatnonzero(np.asarray(committed) < 0).astype(np.int64)
    return idx, np.ascontiguousarray(np.asarray(begin, dtype=np.int64)[idx])


def offset_bounds(begin, end, committed, partition_id, lag=None):
    """What a marshaller that walks every partition knows for free (Main.java:344-356): (largest end offset, largest partition
    id) -- a lag never exceeds its end offset when no offset of the batch is negative -- or None when an offset or an id IS
    negative (then there is nothing to promise).  With `lag` (the precomputed-lags seam): (largest lag, largest id)."""
    pid = np.asarray(partition_id)
    if pid.size == 0 or int(pid.min()) < 0:
        return None
    if lag is not None:
        lag = np.asarray(lag)
        return None if int(lag.min()) < 0 else (int(lag.max()), int(pid.max()))
    end = np.asarray(end)
    if int(end.min()) < 0:
        return None
    if begin is not None:
        b = np.asarray(begin)
        if b.size and int(b.min()) < 0:
            return None
    return int(end.max()), int(pid.max())


def device_count() -> int:
    n = load().la_device_count()
    if n < 0:
        raise LagAssignError(n, load().la_last_error(None).decode())
    return n


class Context:
    """RAII wrapper of la_ctx (one per assignor instance; not thread-safe).

    ``device_id`` may be an int (one device) or a sequence of device ids (la_create_multi: one shard per
    entry; an id may repeat -- several logical shards on one GPU); ``devices="all"`` takes every device."""

    def __init__(self, device_id=0, flags: int = 0):
        self._lib = load()
        h = ctypes.c_void_p()
        if isinstance(device_id, str):
            if device_id != "all":
                raise ValueError("device_id must be an int, a sequence of ints or 'all'")
            rc = self._lib.la_create_multi(ctypes.byref(h), 0, None, flags)
        elif isinstance(device_id, (list, tuple)):
            ids = (ctypes.c_int * len(device_id))(*device_id)
            rc = self._lib.la_create_multi(ctypes.byref(h), len(device_id), ids, flags)
        else:
            rc = self._lib.la_create(ctypes.byref(h), int(device_id), flags)
        if rc != LA_OK:
            raise LagAssignError(rc, self._lib.la_last_error(None).decode())
        self._h = h

    @property
    def shard_count(self) -> int:
        return int(self._lib.la_shard_count(self._h))

    def shard_device(self, i: int) -> int:
        return int(self._lib.la_shard_device(self._h, i))

    def device_features(self, i: int = 0) -> int:
        """LA_FEATURE_* bits of shard i's device."""
        return int(self._lib.la_device_features(self._h, i))

    def last_shard_bounds(self) -> np.ndarray:
        """Topic ranges the last host-buffer assign call gave to its shards (int32 [S + 1])."""
        buf = np.zeros(65, dtype=np.int32)
        s = int(self._lib.la_last_shard_bounds(self._h, _p32(buf), buf.size))
        return buf[: s + 1].copy()

    def host_alloc(self, shape, dtype) -> np.ndarray:
        """A numpy array over pinned host memory from la_host_alloc (freed when the array is collected)."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape))
        p = self._lib.la_host_alloc(self._h, max(1, n * dtype.itemsize))
        if not p:
            raise LagAssignError(LA_ENOMEM, self._lib.la_last_error(self._h).decode())
        lib = self._lib

        class _Owner:
            def __del__(self_inner):
                lib.la_host_free(None, ctypes.c_void_p(p))

        buf = (ctypes.c_char * max(1, n * dtype.itemsize)).from_address(p)
        buf._owner = _Owner()
        return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.la_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int) -> None:
        if rc != LA_OK:
            raise LagAssignError(rc, self._lib.la_last_error(self._h).decode())

    def hint_next_call(self, bounds) -> None:
        """la_hint_next_call: `bounds` = (max_lag, max_partition_id) the caller guarantees for its NEXT host-buffer assign call
        (offset_bounds() computes them the way a marshaller would), or None = no hint (clears a pending one)."""
        if bounds is None:
            self._check(self._lib.la_hint_next_call(self._h, None))
            return
        h = CallHints(ctypes.sizeof(CallHints), LA_HINT_BOUNDS, int(bounds[0]), int(bounds[1]))
        self._check(self._lib.la_hint_next_call(self._h, ctypes.byref(h)))

    def last_launches(self) -> int:
        """Kernel launches the last call on this context enqueued (la_last_launches)."""
        return int(self._lib.la_last_launches(self._h))

    def wake(self) -> None:
        """la_wake: one one-partition rebalance through the real small-call path (waited for) + an empty kernel on every other
        stream -- for the moment a host ENTERS assign(), milliseconds before it has offsets to hand over."""
        self._check(self._lib.la_wake(self._h))

    # -- host-buffer entry points ------------------------------------------------
    def compute_lag(self, begin, end, committed, reset_mode: int, out=None) -> np.ndarray:
        """`out`: a caller-owned contiguous int64[N] for the lags (as for assign_batch)."""
        end, committed = _a64(end), _a64(committed)
        begin = None if begin is None else _a64(begin)
        if out is None:
            out = np.empty_like(end)
        elif not (isinstance(out, np.ndarray) and out.dtype == np.int64 and out.size == end.size and out.flags.c_contiguous):
            raise ValueError("out must be a contiguous int64[N]")
        self._check(self._lib.la_compute_lag(self._h, end.size, _p64(begin), _p64(end), _p64(committed),
                                             reset_mode, _p64(out)))
        return out

    def assign_batch(self, part_off, partition_id, begin, end, committed, reset_mode: int,
                     cons_off, cons_rank, want_totals: bool = True, out=None, keep_on_device: bool = False
                     ) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """`out` = (out_partition int32[N], out_member_rank int32[N], out_total_lag int64[K] or None): caller-owned
        result buffers to reuse across calls (fresh numpy arrays are page-faulted in by the D2H copy, which
        doubles the time of a 25.6 M-partition call)."""
        part_off, cons_off = _a64(part_off), _a64(cons_off)
        partition_id, cons_rank = _a32(partition_id), _a32(cons_rank)
        end, committed = _a64(end), _a64(committed)
        begin = None if begin is None else _a64(begin)
        if keep_on_device:
            # results stay on the device for group_last_by_member(); only the totals come back
            out_p = out_m = None
            out_t = np.zeros(cons_rank.size, dtype=np.int64) if want_totals else None
        elif out is not None:
            out_p, out_m, out_t = _check_out3(out, partition_id.size, cons_rank.size)
        else:
            out_p = np.empty(partition_id.size, dtype=np.int32)
            out_m = np.empty(partition_id.size, dtype=np.int32)
            out_t = np.zeros(cons_rank.size, dtype=np.int64) if want_totals else None
        self._check(self._lib.la_assign_batch(self._h, part_off.size - 1, _p64(part_off), _p32(partition_id),
                                              _p64(begin), _p64(end), _p64(committed), reset_mode,
                                              _p64(cons_off), _p32(cons_rank), _p32(out_p), _p32(out_m),
                                              _p64(out_t)))
        return out_p, out_m, out_t

    def assign_batch_sparse(self, part_off, partition_id, end, committed, reset_mode: int, none_index, none_begin,
                            cons_off, cons_rank, want_totals: bool = True, out=None, keep_on_device: bool = False):
        """la_assign_batch_sparse: `begin` only for the partitions listed in none_index (ascending positions)."""
        part_off, cons_off = _a64(part_off), _a64(cons_off)
        partition_id, cons_rank = _a32(partition_id), _a32(cons_rank)
        end, committed = _a64(end), _a64(committed)
        none_index = None if none_index is None else _a64(none_index)
        none_begin = None if none_begin is None else _a64(none_begin)
        n_none = 0 if none_index is None else none_index.size
        if keep_on_device:
            out_p = out_m = None
            out_t = np.zeros(cons_rank.size, dtype=np.int64) if want_totals else None
        elif out is not None:
            out_p, out_m, out_t = _check_out3(out, partition_id.size, cons_rank.size)
        else:
            out_p = np.empty(partition_id.size, dtype=np.int32)
            out_m = np.empty(partition_id.size, dtype=np.int32)
            out_t = np.zeros(cons_rank.size, dtype=np.int64) if want_totals else None
        self._check(self._lib.la_assign_batch_sparse(self._h, part_off.size - 1, _p64(part_off), _p32(partition_id),
                                                     _p64(end), _p64(committed), reset_mode, n_none, _p64(none_index),
                                                     _p64(none_begin), _p64(cons_off), _p32(cons_rank), _p32(out_p),
                                                     _p32(out_m), _p64(out_t)))
        return out_p, out_m, out_t

    def assign_batch_grouped_sparse(self, part_off, partition_id, end, committed, reset_mode: int, none_index, none_begin,
                                    cons_off, cons_rank, n_members: int, want_totals: bool = True, want_topic: bool = True, out=None):
        """la_assign_batch_grouped_sparse -> (member_off, grouped_topic or None, grouped_partition, totals or None).
        `out`: caller-owned buffers of those four (None entries: not wanted), as for assign_batch_grouped."""
        part_off, cons_off = _a64(part_off), _a64(cons_off)
        partition_id, cons_rank = _a32(partition_id), _a32(cons_rank)
        end, committed = _a64(end), _a64(committed)
        none_index = None if none_index is None else _a64(none_index)
        none_begin = None if none_begin is None else _a64(none_begin)
        n_none = 0 if none_index is None else none_index.size
        if out is not None:
            off, g_t, g_p, out_t = _check_out_grouped(out, n_members, partition_id.size, cons_rank.size)
        else:
            off = np.zeros(n_members + 1, dtype=np.int64)
            g_t = np.empty(partition_id.size, dtype=np.int32) if want_topic else None
            g_p = np.empty(partition_id.size, dtype=np.int32)
            out_t = np.zeros(cons_rank.size, dtype=np.int64) if want_totals else None
        self._check(self._lib.la_assign_batch_grouped_sparse(self._h, part_off.size - 1, _p64(part_off), _p32(partition_id),
                                                             _p64(end), _p64(committed), reset_mode, n_none,
                                                             _p64(none_index), _p64(none_begin), _p64(cons_off),
                                                             _p32(cons_rank), n_members, _p64(off), _p32(g_t), _p32(g_p),
                                                             _p64(out_t)))
        return off, g_t, g_p, out_t

    def assign_batch_lags(self, part_off, partition_id, lag, cons_off, cons_rank, want_totals: bool = True,
                          keep_on_device: bool = False, out=None
                          ) -> Tuple[Optional[np.ndarray], Optional[np.ndarray], Optional[np.ndarray]]:
        """keep_on_device: the results stay on the device for group_last_by_member() (None, None, totals come back).
        out: caller-owned (int32[N], int32[N], int64[K] or None) result buffers, as for assign_batch."""
        part_off, cons_off = _a64(part_off), _a64(cons_off)
        partition_id, cons_rank, lag = _a32(partition_id), _a32(cons_rank), _a64(lag)
        if out is not None and not keep_on_device:
            out_p, out_m, out_t = _check_out3(out, partition_id.size, cons_rank.size)
        else:
            out_p = None if keep_on_device else np.empty(partition_id.size, dtype=np.int32)
            out_m = None if keep_on_device else np.empty(partition_id.size, dtype=np.int32)
            out_t = np.zeros(cons_rank.size, dtype=np.int64) if want_totals else None
        self._check(self._lib.la_assign_batch_lags(self._h, part_off.size - 1, _p64(part_off),
                                                   _p32(partition_id), _p64(lag), _p64(cons_off),
                                                   _p32(cons_rank), _p32(out_p), _p32(out_m), _p64(out_t)))
        return out_p, out_m, out_t

    def assign_batch_grouped(self, part_off, partition_id, begin, end, committed, reset_mode: int, cons_off, cons_rank,
                             n_members: int, want_totals: bool = True, want_topic: bool = True, out=None
                             ) -> Tuple[np.ndarray, Optional[np.ndarray], np.ndarray, Optional[np.ndarray]]:
        """la_assign_batch_grouped: assign and every member's list in ONE call (for a small batch: one upload, one
        download).  Returns (member_off [M+1], grouped_topic [N] or None, grouped_partition [N], totals [K] or None).
        `out` = caller-owned (member_off int64[M+1], grouped_topic int32[N] or None, grouped_partition int32[N], totals int64[K]
        or None) to reuse across calls; its None entries replace want_topic / want_totals."""
        part_off, cons_off = _a64(part_off), _a64(cons_off)
        partition_id, cons_rank = _a32(partition_id), _a32(cons_rank)
        end, committed = _a64(end), _a64(committed)
        begin = None if begin is None else _a64(begin)
        if out is not None:
            off, g_t, g_p, out_t = _check_out_grouped(out, n_members, partition_id.size, cons_rank.size)
        else:
            off = np.zeros(n_members + 1, dtype=np.int64)
            g_t = np.empty(partition_id.size, dtype=np.int32) if want_topic else None
            g_p = np.empty(partition_id.size, dtype=np.int32)
            out_t = np.zeros(cons_rank.size, dtype=np.int64) if want_totals else None
        self._check(self._lib.la_assign_batch_grouped(self._h, part_off.size - 1, _p64(part_off), _p32(partition_id),
                                                      _p64(begin), _p64(end), _p64(committed), reset_mode,
                                                      _p64(cons_off), _p32(cons_rank), n_members, _p64(off), _p32(g_t),
                                                      _p32(g_p), _p64(out_t)))
        return off, g_t, g_p, out_t

    def group_by_member(self, part_off, out_partition, out_member_rank, n_members: int
                        ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(member_off [M+1], grouped_topic [N], grouped_partition [N]): every member's list in the
        reference's order; entries before member_off[0] belong to topics without consumers."""
        part_off = _a64(part_off)
        out_partition, out_member_rank = _a32(out_partition), _a32(out_member_rank)
        off = np.zeros(n_members + 1, dtype=np.int64)
        g_t = np.empty(out_partition.size, dtype=np.int32)
        g_p = np.empty(out_partition.size, dtype=np.int32)
        self._check(self._lib.la_group_by_member(self._h, part_off.size - 1, _p64(part_off), _p32(out_partition),
                                                 _p32(out_member_rank), n_members, _p64(off), _p32(g_t), _p32(g_p)))
        return off, g_t, g_p

    def group_last_by_member(self, n_partitions: int, n_members: int, out=None
                             ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """group_by_member on the results the last assign_batch / assign_batch_lags call left on the device
        (give that call keep_on_device=True to skip the download of the ungrouped arrays).
        `out` = (member_off int64[M+1], grouped_topic int32[N], grouped_partition int32[N]): caller-owned arrays to
        reuse across calls (pinned ones from host_alloc, for instance), as for assign_batch."""
        if out is not None:
            off, g_t, g_p = out
            if (off.dtype != np.int64 or off.size != n_members + 1 or g_t.dtype != np.int32 or g_p.dtype != np.int32 or
                    g_t.size != n_partitions or g_p.size != n_partitions or
                    not (off.flags.c_contiguous and g_t.flags.c_contiguous and g_p.flags.c_contiguous)):
                raise ValueError("out buffers must be contiguous int64[M+1], int32[N], int32[N]")
        else:
            off = np.zeros(n_members + 1, dtype=np.int64)
            g_t = np.empty(n_partitions, dtype=np.int32)
            g_p = np.empty(n_partitions, dtype=np.int32)
        self._check(self._lib.la_group_last_by_member(self._h, n_members, _p64(off), _p32(g_t), _p32(g_p)))
        return off, g_t, g_p

    def group_by_member_device(self, n_topics: int, n_partitions: int, d_part_off: int, d_out_partition: int,
                               d_out_member_rank: int, n_members: int, d_member_off: int, d_grouped_topic: int,
                               d_grouped_partition: int, stream: int = 0, shard: int = 0) -> None:
        self._check(self._lib.la_group_by_member_device_on(self._h, shard, n_topics, n_partitions, d_part_off,
                                                           d_out_partition, d_out_member_rank, n_members,
                                                           d_member_off, d_grouped_topic, d_grouped_partition,
                                                           ctypes.c_void_p(stream)))

    def member_loads_device(self, n_partitions: int, d_out_member_rank: int, n_consumers: int, d_cons_rank: int,
                            d_out_total_lag: int, n_members: int, d_member_partitions: int, d_member_lag: int,
                            d_unassigned: int = 0, stream: int = 0, shard: int = 0) -> None:
        """la_member_loads_device_on: per-member partition counts (int64[M]), total lags (int64[M], Java long sums) and the
        number of unassigned partitions (int64[1]) of an assignment, device addresses as ints (0 = NULL: either half --
        d_out_member_rank with its two outputs, d_cons_rank / d_out_total_lag with d_member_lag -- may be left out).
        Enqueued on `stream`; sync() reports a rank out of range.  sharding.member_loads_numpy is the same on the host."""
        fn = getattr(self._lib, "la_member_loads_device_on", None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no la_member_loads_device_on")

        def p(x):
            return ctypes.c_void_p(int(x)) if x else None

        self._check(fn(self._h, shard, n_partitions, p(d_out_member_rank), n_consumers, p(d_cons_rank), p(d_out_total_lag),
                       n_members, p(d_member_partitions), p(d_member_lag), p(d_unassigned), ctypes.c_void_p(stream)))

    def assignment_moves_device(self, args: MovesArgs, stream: int = 0, shard: int = 0) -> None:
        """la_assignment_moves_device_on: who moved between the previous and the current assignment of one layout -- the previous
        owner of every entry in today's ranks (int32[N]), moved entries per topic (int64[T]), gained / lost per member
        (int64[M]) and the moved total (int64[1]); each output may be left out.  Enqueued on `stream`; sync() reports duplicate or
        missing ids, ranks out of range (LA_EINVAL) and topics over a hint within MOVES_LDS_MAX_PARTITIONS (LA_ESHAPE).
        sharding.assignment_moves_numpy is the same on the host.
        With args.d_prev_part_off the previous assignment has a layout of its own (n_prev_topics, n_prev_partitions,
        d_prev_topic: today's topic -> its previous topic or -1): a partition without a previous entry is ADDED
        (d_prev_owner = LA_MOVES_NO_PREVIOUS, d_topic_added, d_added, gained), a previous entry nobody matched is REMOVED
        (d_topic_removed, d_removed, lost), and a missing id is no error.  sharding.assignment_moves_layouts_numpy is that
        form on the host."""
        fn = getattr(self._lib, "la_assignment_moves_device_on", None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no la_assignment_moves_device_on")
        if not args.struct_size:
            args.struct_size = ctypes.sizeof(MovesArgs)
        self._check(fn(self._h, shard, ctypes.byref(args), ctypes.c_void_p(stream)))

    def verify_assignment_device(self, batch: Optional[DeviceBatch], d_topic_verdict: int, d_summary: int, stream: Optional[int] = None,
                                 shard: Optional[int] = None) -> None:
        """la_verify_assignment_device[_on]: certifies the results `batch` points at against its inputs -- the struct an assign
        call took, verified behind it on the same stream without a sync, or any arrays of that layout.  d_topic_verdict (int32[T])
        reads 0 per certified topic, otherwise a mask of LA_VERDICT_*; d_summary (int64[4]) = topics failed, topics unchecked,
        the lowest index of each or -1.  Device addresses as ints, either may be 0 (NULL).  A non-zero verdict is data: sync()
        raises only for offsets that leave the arrays or a topic over its hint (LA_ESHAPE).  stream None = HIP's default
        stream; shard None = the form without a shard argument.  sharding.verify_assignment_numpy is the same on the host.

        A topic of more than VERIFY_MAX_PARTITIONS partitions or VERIFY_MAX_CONSUMERS consumers reads LA_VERDICT_UNCHECKED unless
        batch.flags carries LA_FLAG_VERIFY_LARGE.  With the flag batch.h_part_off / h_cons_off are required (LA_EINVAL without
        them, or when they do not ascend inside the arrays): the library lists those topics from the HOST offsets and verifies
        them through tables in device memory, verdict and summary as for any other topic (the yardstick with max_partitions /
        max_consumers raised); a topic whose host and device offsets disagree reads UNCHECKED and sync() raises LA_ESHAPE.  The
        flagged call reads host memory and may allocate on first use (LA_ENOMEM, nothing enqueued), so it is not capturable in a
        graph; it enqueues at most VERIFY_MAX_LAUNCHES kernels whatever the number and size of the large topics, and without a
        large topic what the unflagged call enqueues."""
        name = "la_verify_assignment_device" if shard is None else "la_verify_assignment_device_on"
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no %s" % name)

        def p(x):
            return ctypes.c_void_p(int(x)) if x else None

        b = ctypes.byref(batch) if batch is not None else None
        head = (self._h,) if shard is None else (self._h, int(shard))
        self._check(fn(*head, b, p(d_topic_verdict), p(d_summary), ctypes.c_void_p(stream or 0)))

    def cooperative_adjust_device(self, args: CoopArgs, stream: int = 0) -> None:
        """la_cooperative_adjust_device (shard 0 of the context): the target assignment (results of an assign call) against every member's owned list
        (d_owned_member_off int64[M+1], d_owned_topic / d_owned_partition int32[n_owned]: the layout group_by_member_device
        writes) -- the previous owner of every entry (int32[N]), the adjusted ranks with every partition that changes hands
        between two live members withheld as -1 (int32[N]), kept / fresh / pending / release per member (int64[M]), withheld
        per topic (int64[T]) and the summary kept, fresh, withheld, dropped, stale, followup (int64[6]); each output may be left
        out.  Enqueued on `stream`, at most COOP_MAX_LAUNCHES kernels; sync() reports a target rank or owned topic out of range and
        a (topic, id) claimed twice (LA_EINVAL), offsets that do not ascend inside their arrays (LA_ESHAPE).
        sharding.cooperative_adjust_numpy is the same on the host."""
        fn = getattr(self._lib, "la_cooperative_adjust_device", None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no la_cooperative_adjust_device")
        if not args.struct_size:
            args.struct_size = ctypes.sizeof(CoopArgs)
        self._check(fn(self._h, ctypes.byref(args), ctypes.c_void_p(stream)))

    def sticky_ties_device(self, batch: DeviceBatch, args: StickyArgs, stream: int = 0, shard: int = 0) -> None:
        """la_sticky_ties_device: the assignment `batch` points at (the struct an assign call took, inputs and results) with the
        partitions of every run of equal lag re-matched to their previous owners, args.d_prev_owner (int32[N]: what
        assignment_moves_device / cooperative_adjust_device write) -- args.d_sticky_partition (int32[N]) takes the place of
        batch.d_out_partition, the ranks and totals stay as they are; d_topic_kept / d_topic_saved (int64[T]) and d_summary
        (int64[4]: kept before, kept after, topics changed, topics passed through) may be left out.  Enqueued on `stream`, at most
        one kernel; sync() reports duplicate or foreign ids (LA_EINVAL), a topic over its hint and offsets that leave the arrays
        (LA_ESHAPE).  A topic of more than VERIFY_MAX_PARTITIONS partitions is passed through -- unless batch.flags carries
        LA_FLAG_STICKY_LARGE (batch.h_part_off then required): such topics, up to STICKY_GLOBAL_MAX_PARTITIONS partitions, are
        re-matched through tables in device memory in at most STICKY_GLOBAL_LAUNCHES more launches; that call reads host memory
        and may allocate.  The C ABI has the call on shard 0 only: another shard needs a library that exports
        la_sticky_ties_device_on.  sharding.sticky_ties_numpy, with max_partitions=STICKY_ANY_SIZE for the flagged call, is the
        same on the host."""
        name = "la_sticky_ties_device" if not shard else "la_sticky_ties_device_on"
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no %s" % name)
        if not args.struct_size:
            args.struct_size = ctypes.sizeof(StickyArgs)
        head = (self._h,) if not shard else (self._h, int(shard))
        self._check(fn(*head, ctypes.byref(batch) if batch is not None else None, ctypes.byref(args), ctypes.c_void_p(stream)))

    def cooperative_round_device(self, args: CoopRoundArgs, stream: int = 0) -> None:
        """la_cooperative_round_device (shard 0 of the context): cooperative_adjust_device on args.adjust -- every one of its
        outputs optional -- and every member's list of the adjusted assignment (member_off int64[M+1], grouped_topic int32[N] or
        0, grouped_partition int32[N]): what group_by_member_device writes for the adjusted ranks, whether args.adjust wants
        them or not, so the lists of one round can be the owned arrays of the next as they lie.  Within COOP_SMALL_ENTRIES /
        _OWNED / _MEMBERS / _TOPICS it is ONE kernel launch without memset, allocation or scratch; otherwise, or with
        args.flags = LA_COOP_FORCE_TABLE, the table form followed by the grouping.  Errors as for cooperative_adjust_device.
        sharding.cooperative_round_numpy is the same on the host."""
        fn = getattr(self._lib, "la_cooperative_round_device", None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no la_cooperative_round_device")
        if not args.struct_size:
            args.struct_size = ctypes.sizeof(CoopRoundArgs)
        self._check(fn(self._h, ctypes.byref(args), ctypes.c_void_p(stream)))

    def cooperative_round_sticky_device(self, batch: DeviceBatch, args: CoopStickyArgs, stream: int = 0) -> None:
        """la_cooperative_round_sticky_device (shard 0 of the context): the cooperative round on the STICKY order in one call --
        bit for bit what cooperative_adjust_device (for d_prev_owner), sticky_ties_device and cooperative_round_device with
        d_sticky_partition in place of d_out_partition write when chained on one stream.  `batch` is the struct an assign call
        took, read as sticky_ties_device reads it; the target is the batch's.  args.d_sticky_partition (int32[N]) is required,
        d_topic_kept / d_topic_saved (int64[T]) and d_sticky_summary (int64[4]) may be left out, and so may each of the eight
        adjust outputs; the round's outputs describe the sticky order.  Within COOP_STICKY_ENTRIES / _OWNED / _MEMBERS / _TOPICS
        it is ONE kernel launch without memset, allocation or scratch; otherwise, or with args.flags = LA_COOP_FORCE_TABLE, the
        chain itself.  Errors are the union of the three calls'.  LA_FLAG_STICKY_LARGE in batch.flags (with batch.h_part_off)
        reaches the chain's sticky step: topics of more than VERIFY_MAX_PARTITIONS partitions are re-matched as sticky_ties_device
        describes.  sharding.cooperative_round_sticky_numpy (max_partitions=STICKY_ANY_SIZE for the flagged call) is the same on
        the host."""
        fn = getattr(self._lib, "la_cooperative_round_sticky_device", None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no la_cooperative_round_sticky_device")
        if not args.struct_size:
            args.struct_size = ctypes.sizeof(CoopStickyArgs)
        self._check(fn(self._h, ctypes.byref(batch) if batch is not None else None, ctypes.byref(args), ctypes.c_void_p(stream)))

    def assign_pinned_device(self, batch: DeviceBatch, args: PinnedArgs, stream: int = 0) -> None:
        """la_assign_pinned_device (shard 0 of the context): the PINNED assignment of `batch` (the struct an assign call takes)
        against every member's owned list (args.d_owned_member_off int64[M+1], d_owned_topic / d_owned_partition
        int32[n_owned]) -- a partition that a consumer of its topic owns stays with it, every consumer's bin starts from what it
        holds, only the other partitions are dealt out by the reference's rule.  Writes batch.d_out_partition /
        d_out_member_rank / d_out_total_lag in the layout of an assign result, args.d_topic_free (int64[T]) and args.d_summary
        (int64[4]: pinned, free, foreign, stale), the last three optional.  Enqueued on `stream`, at most PINNED_MAX_LAUNCHES
        kernels; sync() reports an unsorted cons_rank segment, an owned topic out of range and a (topic, id) claimed twice
        (LA_EINVAL), offsets that do not ascend inside their arrays and a topic over PINNED_MAX_PARTITIONS /
        PINNED_MAX_CONSUMERS (LA_ESHAPE; such a topic is left untouched).  sharding.assign_pinned_numpy is the same on the host."""
        fn = getattr(self._lib, "la_assign_pinned_device", None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no la_assign_pinned_device")
        if not args.struct_size:
            args.struct_size = ctypes.sizeof(PinnedArgs)
        self._check(fn(self._h, ctypes.byref(batch) if batch is not None else None, ctypes.byref(args), ctypes.c_void_p(stream)))

    def cooperative_round(self, part_off, out_partition, out_member_rank, n_members: int, owned_off, owned_topic, owned_partition,
                          force_table: bool = False) -> CoopRound:
        """la_cooperative_round: the cooperative round on host arrays (numpy in, a CoopRound of numpy arrays out) -- the target
        (part_off, out_partition, out_member_rank) against every member's owned list (owned_off int64[M+1], owned_topic /
        owned_partition; all three None when nobody owns anything).  One copy each way, waited for; raises what sync() would.
        sharding.cooperative_round_numpy is the same on the host."""
        fn = getattr(self._lib, "la_cooperative_round", None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no la_cooperative_round")
        part_off, out_partition, out_member_rank = _a64(part_off), _a32(out_partition), _a32(out_member_rank)
        m, t, n = int(n_members), part_off.size - 1, out_partition.size
        if t < 0 or out_member_rank.size != n:
            raise ValueError("part_off is empty, or out_partition and out_member_rank differ in length")
        owned_topic = _a32(owned_topic if owned_topic is not None else [])
        owned_partition = _a32(owned_partition if owned_partition is not None else [])
        if owned_partition.size != owned_topic.size:
            raise ValueError("owned_topic and owned_partition differ in length")
        if owned_off is None:
            if owned_topic.size:
                raise ValueError("owned entries without owned_off")
        else:
            owned_off = _a64(owned_off)
            if owned_off.size != m + 1:
                raise ValueError("owned_off must hold n_members + 1 offsets")
        out = CoopRound(np.empty(n, np.int32), np.empty(n, np.int32), np.empty(m, np.int64), np.empty(m, np.int64),
                        np.empty(m, np.int64), np.empty(m, np.int64), np.empty(t, np.int64), np.empty(6, np.int64),
                        np.empty(m + 1, np.int64), np.empty(n, np.int32), np.empty(n, np.int32))
        p = lambda a: a.ctypes.data if a is not None and a.size else None
        r = CoopRoundArgs()
        r.struct_size, r.flags = ctypes.sizeof(CoopRoundArgs), LA_COOP_FORCE_TABLE if force_table else 0
        a = r.adjust
        a.struct_size = ctypes.sizeof(CoopArgs)
        a.n_topics, a.n_partitions, a.n_members, a.n_owned = t, n, m, owned_topic.size
        a.d_part_off, a.d_out_partition, a.d_out_member_rank = part_off.ctypes.data, p(out_partition), p(out_member_rank)
        a.d_owned_member_off, a.d_owned_topic, a.d_owned_partition = p(owned_off), p(owned_topic), p(owned_partition)
        a.d_prev_owner, a.d_coop_member_rank = p(out.prev_owner), p(out.coop_member_rank)
        a.d_member_kept, a.d_member_fresh, a.d_member_pending = p(out.kept), p(out.fresh), p(out.pending)
        a.d_member_release, a.d_topic_withheld, a.d_summary = p(out.release), p(out.topic_withheld), out.summary.ctypes.data
        r.member_off, r.grouped_topic, r.grouped_partition = out.member_off.ctypes.data, p(out.grouped_topic), p(out.grouped_partition)
        self._check(fn(self._h, ctypes.byref(r)))
        return out

    def assign_batch_cooperative(self, part_off, partition_id, cons_off, cons_rank, n_members: int, owned_off, owned_topic,
                                 owned_partition, *, lag=None, begin=None, end=None, committed=None, reset_mode: int = 0,
                                 none_index=None, none_begin=None, force_table: bool = False,
                                 out: Optional[AssignCoop] = None, pinned: bool = False, pinned_large: bool = False) -> AssignCoop:
        """la_assign_batch_cooperative: a COOPERATIVE rebalance in one call -- the assign call (`lag`: assign_batch_lags; `begin`:
        assign_batch; neither: assign_batch_sparse with none_index / none_begin) and cooperative_round on its result against
        every member's owned list (owned_off int64[M+1], owned_topic / owned_partition; all three None when nobody owns
        anything).  Returns an AssignCoop; `out` = caller-owned buffers in that shape, None entries are not computed.  A small
        call is zero-copy with the round as its last launch; the target stays on the device for group_last_by_member().
        sharding.assign_cooperative_numpy is the same on the host.
        pinned: LA_COOP_PINNED -- the target is the PINNED assignment (assign_pinned_device: what a subscriber owns stays with
        it, only the rest is dealt out), the follow-up form that settles; one copy each way through the cooperative staging
        buffers, no fused form, a topic over PINNED_MAX_PARTITIONS / PINNED_MAX_CONSUMERS raises LA_ESHAPE at the call.
        sharding.assign_cooperative_numpy with assign = the first three results of sharding.assign_pinned_numpy is the same on
        the host.
        pinned_large: LA_COOP_PINNED_LARGE, only with pinned (LA_EINVAL otherwise) -- topics of up to PINNED_LARGE_MAX_PARTITIONS
        partitions are taken (assign_pinned_device with LA_FLAG_PINNED_LARGE); the host form is assign_pinned_numpy with
        max_partitions=sharding.PINNED_ANY_SIZE."""
        fn = getattr(self._lib, "la_assign_batch_cooperative", None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no la_assign_batch_cooperative")
        g = AssignCoopArgs()
        out = self._fill_assign_coop(g, part_off, partition_id, cons_off, cons_rank, n_members, owned_off, owned_topic, owned_partition,
                                     lag, begin, end, committed, reset_mode, none_index, none_begin, force_table, out)
        if pinned:
            g.flags |= LA_COOP_PINNED
        if pinned_large:
            g.flags |= LA_COOP_PINNED_LARGE
        self._check(fn(self._h, ctypes.byref(g)))
        return out

    def assign_batch_cooperative_sticky(self, part_off, partition_id, cons_off, cons_rank, n_members: int, owned_off, owned_topic,
                                        owned_partition, *, lag=None, begin=None, end=None, committed=None, reset_mode: int = 0,
                                        none_index=None, none_begin=None, force_table: bool = False,
                                        out: Optional[AssignSticky] = None, large: bool = False) -> AssignSticky:
        """la_assign_batch_cooperative_sticky: assign_batch_cooperative with the round on the STICKY order (partitions of equal
        lag stay with their previous owner).  Same inputs; returns an AssignSticky: .coop.out_partition / out_member_rank /
        totals describe the TARGET, every other entry of .coop and sticky_partition / topic_kept / topic_saved / sticky_summary
        the sticky order; `out` = caller-owned buffers in that shape (None entries of out.coop are not computed).
        large: LA_COOP_STICKY_LARGE -- topics of more than VERIFY_MAX_PARTITIONS partitions are re-matched too instead of being
        passed through.  A small call (within COOP_STICKY_ENTRIES / _OWNED / _MEMBERS / _TOPICS, without force_table) is zero-copy
        with the sticky round as its last launch, like assign_batch_cooperative; LA_NO_FUSED_STICKY=1 in the environment sends
        every call through the general form.  sharding.assign_cooperative_sticky_numpy (max_partitions=STICKY_ANY_SIZE for
        large) is the same on the host."""
        fn = getattr(self._lib, "la_assign_batch_cooperative_sticky", None)
        if fn is None:
            raise LagAssignError(LA_EINVAL, "this liblagassign.so has no la_assign_batch_cooperative_sticky")
        a = AssignStickyArgs()
        a.struct_size = ctypes.sizeof(AssignStickyArgs)
        coop = self._fill_assign_coop(a.coop, part_off, partition_id, cons_off, cons_rank, n_members, owned_off, owned_topic,
                                      owned_partition, lag, begin, end, committed, reset_mode, none_index, none_begin, force_table,
                                      None if out is None else out.coop)
        if large:
            a.coop.flags |= LA_COOP_STICKY_LARGE
        n, t = coop.grouped_partition.size, _a64(part_off).size - 1
        if out is None:
            out = AssignSticky(coop, np.empty(n, np.int32), np.empty(t, np.int64), np.empty(t, np.int64), np.empty(4, np.int64))
        elif (out.sticky_partition.dtype, out.sticky_partition.size) != (np.int32, n) or \
                any((x.dtype, x.size) != (np.int64, k) for x, k in ((out.topic_kept, t), (out.topic_saved, t), (out.sticky_summary, 4))):
            raise ValueError("out: sticky_partition int32[N], topic_kept / topic_saved int64[T], sticky_summary int64[4]")
        p = lambda x: x.ctypes.data if x.size else None
        a.sticky_partition, a.topic_kept, a.topic_saved = p(out.sticky_partition), p(out.topic_kept), p(out.topic_saved)
        a.sticky_summary = out.sticky_summary.ctypes.data
        self._check(fn(self._h, ctypes.byref(a)))
        return out

    def _fill_assign_coop(self, g, part_off, partition_id, cons_off, cons_rank, n_members, owned_off, owned_topic, owned_partition,
                          lag, begin, end, committed, reset_mode, none_index, none_begin, force_table, out):
        """Fills the AssignCoopArgs `g` from numpy arrays (kept alive on self until the next call) -> the AssignCoop of outputs."""
        part_off, cons_off = _a64(part_off), _a64(cons_off)
        partition_id, cons_rank = _a32(partition_id), _a32(cons_rank)
        m, t, n, k = int(n_members), part_off.size - 1, partition_id.size, cons_rank.size
        if t < 0 or cons_off.size != t + 1:
            raise ValueError("part_off is empty, or part_off and cons_off differ in length")
        lag, begin = (None if lag is None else _a64(lag)), (None if begin is None else _a64(begin))
        end, committed = (None if end is None else _a64(end)), (None if committed is None else _a64(committed))
        none_index = None if none_index is None else _a64(none_index)
        none_begin = None if none_begin is None else _a64(none_begin)
        owned_topic = _a32(owned_topic if owned_topic is not None else [])
        owned_partition = _a32(owned_partition if owned_partition is not None else [])
        if owned_partition.size != owned_topic.size:
            raise ValueError("owned_topic and owned_partition differ in length")
        if owned_off is None:
            if owned_topic.size:
                raise ValueError("owned entries without owned_off")
        else:
            owned_off = _a64(owned_off)
            if owned_off.size != m + 1:
                raise ValueError("owned_off must hold n_members + 1 offsets")
        if out is not None:
            out = _check_out_coop(out, m, n, k, t)
        else:
            out = AssignCoop(np.empty(n, np.int32), np.empty(n, np.int32), np.zeros(k, np.int64),
                             np.empty(n, np.int32), np.empty(n, np.int32), np.empty(m, np.int64), np.empty(m, np.int64),
                             np.empty(m, np.int64), np.empty(m, np.int64), np.empty(t, np.int64), np.empty(6, np.int64),
                             np.empty(m + 1, np.int64), np.empty(n, np.int32), np.empty(n, np.int32))
        p = lambda a: a.ctypes.data if a is not None and a.size else None
        g.struct_size, g.flags = ctypes.sizeof(AssignCoopArgs), LA_COOP_FORCE_TABLE if force_table else 0
        g.n_topics, g.reset_mode = t, reset_mode
        g.part_off, g.partition_id, g.lag = part_off.ctypes.data, p(partition_id), p(lag)
        if lag is not None and not lag.size:
            g.lag = lag.ctypes.data                    # (lags mode is chosen by the pointer, also for an empty batch)
        g.begin_off, g.end_off, g.committed_off = p(begin), p(end), p(committed)
        g.n_none = 0 if none_index is None else none_index.size
        g.none_index, g.none_begin = p(none_index), p(none_begin)
        g.cons_off, g.cons_rank = cons_off.ctypes.data, p(cons_rank)
        g.n_members, g.n_owned = m, owned_topic.size
        g.owned_member_off, g.owned_topic, g.owned_partition = p(owned_off), p(owned_topic), p(owned_partition)
        g.member_off, g.grouped_topic, g.grouped_partition = out.member_off.ctypes.data, p(out.grouped_topic), p(out.grouped_partition)
        g.out_total_lag, g.out_partition, g.out_member_rank = p(out.totals), p(out.out_partition), p(out.out_member_rank)
        g.prev_owner, g.coop_member_rank = p(out.prev_owner), p(out.coop_member_rank)
        g.member_kept, g.member_fresh, g.member_pending = p(out.kept), p(out.fresh), p(out.pending)
        g.member_release, g.topic_withheld = p(out.release), p(out.topic_withheld)
        g.summary = None if out.summary is None else out.summary.ctypes.data
        self._inputs = (part_off, partition_id, cons_off, cons_rank, lag, begin, end, committed, none_index, none_begin, owned_off,
                        owned_topic, owned_partition)
        return out

    # -- device-resident entry point ------------------------------------------------
    def assign_batch_device(self, batch: DeviceBatch, stream: int = 0, shard: int = 0) -> None:
        """Enqueue on `stream` (a hipStream_t handle as an int; 0 = HIP's default stream) of shard `shard`'s device."""
        self._check(self._lib.la_assign_batch_device_on(self._h, shard, ctypes.byref(batch), ctypes.c_void_p(stream)))

    def sync(self, stream: int = 0, shard: int = 0) -> None:
        self._check(self._lib.la_sync_on(self._h, shard, ctypes.c_void_p(stream)))

    def allgather_results(self, count: int, d_send, d_recv) -> None:
        """la_allgather_results: d_send / d_recv are lists of device pointers (ints), one per shard."""
        n = self.shard_count
        send = (ctypes.c_void_p * n)(*[ctypes.c_void_p(int(x)) for x in d_send])
        recv = (ctypes.c_void_p * n)(*[ctypes.c_void_p(int(x)) for x in d_recv])
        self._check(self._lib.la_allgather_results(self._h, count, send, recv))

    def pack_results(self, n: int, d_out_partition: int, d_out_member_rank: int, fmt: WireFormat, d_packed: int,
                     stream: int = 0, shard: int = 0) -> None:
        """la_pack_results_on: n (partition id, member rank) pairs -> n wire elements (device pointers as ints)."""
        self._check(self._lib.la_pack_results_on(self._h, shard, n, ctypes.c_void_p(d_out_partition),
                                                 ctypes.c_void_p(d_out_member_rank), ctypes.byref(fmt),
                                                 ctypes.c_void_p(d_packed), ctypes.c_void_p(stream)))

    def unpack_results(self, n: int, d_packed: int, fmt: WireFormat, d_out_partition: int, d_out_member_rank: int,
                       stream: int = 0, shard: int = 0) -> None:
        """la_unpack_results_on: the reverse."""
        self._check(self._lib.la_unpack_results_on(self._h, shard, n, ctypes.c_void_p(d_packed), ctypes.byref(fmt),
                                                   ctypes.c_void_p(d_out_partition), ctypes.c_void_p(d_out_member_rank),
                                                   ctypes.c_void_p(stream)))

    def allgather_packed(self, count: int, elem_bytes: int, d_send, d_recv) -> None:
        """la_allgather_packed: d_send / d_recv are lists of device pointers (ints), one per shard."""
        n = self.shard_count
        send = (ctypes.c_void_p * n)(*[ctypes.c_void_p(int(x)) for x in d_send])
        recv = (ctypes.c_void_p * n)(*[ctypes.c_void_p(int(x)) for x in d_recv])
        self._check(self._lib.la_allgather_packed(self._h, count, elem_bytes, send, recv))

    def last_pipeline(self) -> int:
        """LA_PIPELINE_* of the last host-buffer assign call."""
        return int(self._lib.la_last_pipeline(self._h))

    def shard_stream(self, shard: int) -> int:
        return int(self._lib.la_shard_stream(self._h, shard) or 0)

    def last_phase_times(self) -> PhaseTimes:
        """Phase times of the large-path topic of the last assign_batch_device call with LA_FLAG_PROFILE."""
        t = PhaseTimes()
        self._check(self._lib.la_last_phase_times(self._h, ctypes.byref(t)))
        return t

    @property
    def stream(self) -> int:
        return int(self._lib.la_stream(self._h) or 0)
