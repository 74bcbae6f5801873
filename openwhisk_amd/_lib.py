"""ctypes binding of libowgs.so (the C ABI in include/owgs.h).

The product path has no CPU fallback: if the HIP library is missing or no MI355X is visible, every constructor
raises.  build() compiles the library in-tree (hipcc --offload-arch=gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
LIB_PATH = os.environ.get("OWGS_LIB") or os.path.join(PKG, "libowgs.so")
HEADER = os.path.join(ROOT, "include", "owgs.h")

OK = 0
EINVAL, ENOMEM, EDEVICE, ERANGE, ENOENT = -22, -12, -5, -34, -2
NONE, THROW_INDEX = -1, -2
NOT_PUBLISHED = -3  # owgs_invoke_activations: out_invoker of an item the gate did not hand to publish
FLAG_OVERLOAD = 1
REL_NOSUCHELEMENT, REL_OVERFLOW, REL_NOENTRY = 1, 2, 4
ACK_FAIL, ACK_JVM, ACK_UNSUPPORTED, ACK_RELEASED, ACK_HEALTH, ACK_NOENTRY, ACK_FORCED_NOENTRY = range(7)
ACK_RESULT = 7  # owgs_process_result_acks: an accepted ResultMessage
ACKF_RESULT, ACKF_RIGHT = 8, 16  # ... and its out_flags bits: carries a result; the result is an object
HEALTHY, UNHEALTHY, UNRESPONSIVE, OFFLINE = 0, 1, 2, 3
EV_PING, EV_SUCCESS, EV_SYSTEM_ERROR, EV_TIMEOUT, EV_STATE_TIMEOUT = range(5)
PING_FAIL, PING_UNSUPPORTED, PING_FED, PING_RANGE = 0, 2, 3, 4  # owgs_process_pings outcomes
HEALTH_MAX_ID = 1 << 24  # OWGS_HEALTH_MAX_ID
NO_DEADLINE = 2**63 - 1  # owgs_next_deadline: nothing armed
NS_INITIAL_CAP = 1024  # OWGS_NS_INITIAL_CAP: namespaces the device counter array holds before it first grows
ADMIT_OK, ADMIT_RATE, ADMIT_CONCURRENT = 0, 1, 2  # owgs_admit_batch verdicts
ADMIT_TRIGGER, ADMIT_RATE_OVERRIDE, ADMIT_CONC_OVERRIDE = 1, 2, 4  # ... and its kind bits
RATE_ABSENT = -2**63  # owgs_rate_state: no record yet
# owgs_throttle_events: the largest event without source and identity pieces, the largest rejection text
EVENT_NAME_MAX = 21
EVENT_MAX_FIXED = len('{"body":{"metricName":"","metricValue":},"eventType":"Metric","source":,,"timestamp":,}') + 21 + 11 + 20
REJECT_TEXT_MAX = len("Too many concurrent requests in flight (count: , allowed: ).") + 11 + 11


class OwgsError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"owgs error {code}: {msg}")
        self.code = code


class owgs_config(C.Structure):
    _fields_ = [
        ("managed_fraction", C.c_double),
        ("blackbox_fraction", C.c_double),
        ("min_memory_bytes", C.c_int64),
        ("cluster_size", C.c_int32),
        ("device", C.c_int32),
        ("rng_seed", C.c_uint64),
    ]


class owgs_replay_io(C.Structure):
    """include/owgs.h: owgs_replay_io (one controller shard of owgs_replay_device_multi)."""
    _fields_ = [("n_batches", C.c_int32), ("acq_off", C.c_void_p), ("act", C.c_void_p),
                ("n_activations", C.c_int64), ("rel_off", C.c_void_p), ("rel_aid", C.c_void_p),
                ("n_releases", C.c_int64), ("seq_base", C.c_uint64), ("out_invoker", C.c_void_p),
                ("out_flags", C.c_void_p), ("rel_flags", C.c_void_p)]


class owgs_msg_batch(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(k, C.c_void_p) for k in (
        "invoker", "tmpl", "aid", "tid", "tid_off", "tid_start", "flags", "content", "content_off", "cause", "trace",
        "trace_off")]


class owgs_publish_io(C.Structure):
    """include/owgs.h: owgs_publish_io (the inputs and the four outputs of owgs_publish_activations)."""
    _fields_ = [("n", C.c_int32), ("action", C.c_void_p), ("seq", C.c_void_p), ("seq_base", C.c_uint64),
                ("aid", C.c_void_p), ("ns", C.c_void_p), ("ticket", C.c_void_p), ("time_limit_ms", C.c_void_p),
                ("now_ms", C.c_int64), ("out_invoker", C.c_void_p), ("out_flags", C.c_void_p),
                ("out_ticket", C.c_void_p), ("out_existed", C.c_void_p)]


class owgs_invoke_io(C.Structure):
    """include/owgs.h: owgs_invoke_io (the gate's and publish's inputs and the nine outputs of owgs_invoke_activations)."""
    _fields_ = [("n", C.c_int32), ("ns", C.c_void_p), ("kind", C.c_void_p), ("t_ms", C.c_void_p),
                ("rate_override", C.c_void_p), ("conc_override", C.c_void_p), ("action", C.c_void_p),
                ("seq", C.c_void_p), ("seq_base", C.c_uint64), ("aid", C.c_void_p), ("ticket", C.c_void_p),
                ("time_limit_ms", C.c_void_p), ("now_ms", C.c_int64), ("out_verdict", C.c_void_p),
                ("out_rate_count", C.c_void_p), ("out_rate_limit", C.c_void_p), ("out_conc_count", C.c_void_p),
                ("out_conc_limit", C.c_void_p), ("out_invoker", C.c_void_p), ("out_flags", C.c_void_p),
                ("out_ticket", C.c_void_p), ("out_existed", C.c_void_p)]


class owgs_event_io(C.Structure):
    """include/owgs.h: owgs_event_io (the identities, the two host regions and what the call writes about them)."""
    _fields_ = [("ident", C.c_void_p), ("ev_out", C.c_void_p), ("ev_cap", C.c_int64), ("ev_off", C.c_void_p),
                ("rej_out", C.c_void_p), ("rej_cap", C.c_int64), ("rej_off", C.c_void_p), ("ev_total", C.c_int64),
                ("rej_total", C.c_int64), ("n_events", C.c_int32), ("n_rejects", C.c_int32)]


class owgs_ack_out(C.Structure):
    """include/owgs.h: owgs_ack_out (the seven output arrays of owgs_process_result_acks)."""
    _fields_ = [(k, C.c_void_p) for k in ("kind", "invoker", "ticket", "flags", "aid", "resp_off", "resp_len")]


class owgs_msg_out(C.Structure):
    """include/owgs.h: owgs_msg_out (the outputs of owgs_serialize_activations as host buffers)."""
    _fields_ = [("n_topics", C.c_int32), ("out", C.c_void_p), ("cap", C.c_int64), ("out_off", C.c_void_p),
                ("out_order", C.c_void_p), ("topic_start", C.c_void_p), ("total", C.c_int64), ("m", C.c_int32)]


def build(verbose: bool = False) -> str:
    """Compile libowgs.so for gfx950 in-tree."""
    out = subprocess.run(["make", "-s", "-C", PKG], capture_output=not verbose, text=True)
    if out.returncode != 0:
        raise RuntimeError(f"libowgs build failed:\n{out.stdout}\n{out.stderr}")
    return LIB_PATH


def header_functions() -> list[str]:
    """Names of every function declared in include/owgs.h."""
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|void|const char\*)\s+(owgs_\w+)\s*\(", src, flags=re.M)))


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OwgsError(EDEVICE, f"{LIB_PATH} is missing: run openwhisk_amd._lib.build() (hipcc, gfx950)")
    # PyTorch-ROCm ships its own HIP runtime: when both are used in one process, torch's must be the one loaded
    # (libowgs.so then binds to it by soname); loading libowgs first leaves torch without a visible device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    i32, u64, P = C.c_int32, C.c_uint64, C.c_void_p
    sig = {
        "owgs_abi_version": (C.c_int, []),
        "owgs_limits": (C.c_int, [P, P]),
        "owgs_create": (C.c_int, [P, P]),
        "owgs_destroy": (None, [P]),
        "owgs_last_error": (C.c_char_p, [P]),
        "owgs_update_invokers": (C.c_int, [P, i32, P, P, P]),
        "owgs_update_cluster": (C.c_int, [P, i32]),
        "owgs_health_events": (C.c_int, [P, i32, P, P, P, P, C.c_int64, i32]),
        "owgs_register_templates": (C.c_int, [P, i32, P, P, P, P, P]),
        "owgs_engine_ms": (C.c_int, [P, P]),
        "owgs_live_resources": (C.c_int, [P]),
        "owgs_resident_stats": (C.c_int, [P, P, i32]),
        "owgs_large_stats": (C.c_int, [P, P, i32]),
        "owgs_set_root_controller": (C.c_int, [P, C.c_char_p, i32]),
        "owgs_serialize_activations": (C.c_int, [P, P, i32, P, C.c_int64, P, P, P, P, P]),
        "owgs_serialize_activations_device": (C.c_int, [P, P, i32, P, C.c_int64, P, P, P, P, P, P]),
        "owgs_publish_activations": (C.c_int, [P, P, P, P, P]),
        "owgs_invoke_activations": (C.c_int, [P, P, P, P, P]),
        "owgs_set_event_source": (C.c_int, [P, C.c_char_p, i32]),
        "owgs_register_event_identities": (C.c_int, [P, i32, P, P, P, P, P]),
        "owgs_throttle_events": (C.c_int, [P, i32, P, P, P, P, P, P, P, P]),
        "owgs_invoke_activations_events": (C.c_int, [P, P, P, P, P, P]),
        "owgs_health_read": (C.c_int, [P, i32, P, P, P, P, P, P]),
        "owgs_process_pings": (C.c_int, [P, i32, P, P, P, C.c_int64, i32, P, P, P, P]),
        "owgs_process_acks_supervised": (C.c_int, [P, i32, P, P, P, P, P, P, C.c_int64, i32, P]),
        "owgs_complete_activations_supervised": (C.c_int, [P, i32, P, P, P, P, P, P, C.c_int64, i32, P]),
        "owgs_process_result_acks": (C.c_int, [P, i32, P, P, P, C.c_int64, i32, P]),
        "owgs_register_actions": (C.c_int, [P, i32, P, P, P, P, P, P, P, P, P, P, P]),
        "owgs_publish_batch": (C.c_int, [P, i32, P, P, u64, P, P]),
        "owgs_release_batch": (C.c_int, [P, i32, P, P, P]),
        "owgs_process_batch": (C.c_int, [P, i32, P, P, P, P, P, P, P, u64, P, P]),
        "owgs_schedule_walks": (C.c_int, [P, i32, P, P, P, P, P, P, P, P, P]),
        "owgs_set_slots": (C.c_int, [P, i32, P]),
        "owgs_set_pool": (C.c_int, [P, i32, i32, P, P]),
        "owgs_read_permits": (C.c_int, [P, P, i32, P]),
        "owgs_read_concurrent": (C.c_int, [P, i32, i32, P, P]),
        "owgs_key_id": (C.c_int, [P, i32]),
        "owgs_map_fill": (C.c_int, [P, P, P, P, P]),
        "owgs_release_actions": (C.c_int, [P, i32, P]),
        "owgs_geometry_selfcheck": (C.c_int, []),
        "owgs_state_info": (C.c_int, [P, P, P, P, P]),
        "owgs_step_sizes": (C.c_int, [P, i32, P, i32, P]),
        "owgs_pairwise_coprime": (C.c_int, [P, i32, P, i32, P]),
        "owgs_set_health_tid": (C.c_int, [P, C.c_int64]),
        "owgs_track_activations": (C.c_int, [P, i32, P, P, P, P, P]),
        "owgs_process_acks": (C.c_int, [P, i32, P, P, P, P, P, P]),
        "owgs_process_acks_device": (C.c_int, [P, i32, P, P, P, P, P, P, P]),
        "owgs_complete_activations": (C.c_int, [P, i32, P, P, P, P, P, P]),
        "owgs_activations_live": (C.c_int, [P, P]),
        "owgs_register_namespaces": (C.c_int, [P, i32, P, P]),
        "owgs_track_activations_ns": (C.c_int, [P, i32, P, P, P, P, P, P]),
        "owgs_active_activations": (C.c_int, [P, i32, P, P]),
        "owgs_activation_totals": (C.c_int, [P, P]),
        "owgs_throttle_batch": (C.c_int, [P, i32, P, P, P, P]),
        "owgs_set_throttle_limits": (C.c_int, [P, i32, i32, i32]),
        "owgs_admit_batch": (C.c_int, [P, i32, P, P, P, P, P, P, P, P, P, P]),
        "owgs_rate_state": (C.c_int, [P, i32, P, i32, P, P]),
        "owgs_set_ack_timeout": (C.c_int, [P, C.c_int64, i32, C.c_int64]),
        "owgs_track_activations_timed": (C.c_int, [P, i32, P, P, P, P, P, P, C.c_int64, P, P]),
        "owgs_expire_activations": (C.c_int, [P, C.c_int64, i32, i32, P, P, P, P, P, P, P]),
        "owgs_next_deadline": (C.c_int, [P, P]),
        "owgs_expiry_stats": (C.c_int, [P, P]),
        "owgs_replay_device": (C.c_int, [P, i32, P, P, C.c_int64, P, P, C.c_int64, u64, P, P, P, P]),
        "owgs_replay_device_multi": (C.c_int, [P, i32, P, P]),
        "owgs_replay_device_span": (C.c_int, [P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, P, P, u64, P, P, P, P]),
        "owgs_replay_device_group": (C.c_int, [P, C.c_int32, P, P, P, P, u64, P, P, P, P, C.c_int64, C.c_int32, P]),
        "owgs_replay": (C.c_int, [P, i32, P, P, P, P, u64, P, P, P]),
        "owgs_snapshot": (C.c_int, [P]),
        "owgs_restore": (C.c_int, [P, P]),
        "owgs_update_health_device": (C.c_int, [P, i32, P, P]),
        "owgs_read_stats": (C.c_int, [P, P, i32]),
        "owgs_selftest": (C.c_int, [P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def live_resources() -> tuple[int, int, int]:
    """What the library holds in this process: (device allocations, pinned host blocks, events + streams)."""
    out = (C.c_int64 * 3)()
    rc = lib().owgs_live_resources(out)
    if rc < 0:
        raise OwgsError(rc, "owgs_live_resources")
    return out[0], out[1], out[2]
