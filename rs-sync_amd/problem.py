"""Python mirror of the reference's ``ISyncProblem`` (src/core/public/rssync.h:9-29).

Method names, argument order, units and the end-exclusive (PreSync) /
end-inclusive (Sync) frame ranges are the reference's.  Everything is a thin
ctypes call into ``librssync_core.so`` through the flat C-ABI declared in
``include/rssync_c.h``; the library is required (no Python or CPU fallback).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class RsSyncError(RuntimeError):
    """A 'panic' of the library (invalid input, device failure) in status mode."""


def library_path():
    """librssync_core.so next to this file.  RSSYNC_LIB names another BUILD of the same library (kernel A/B
    scripts select their variants this way instead of copying over the product .so)."""
    return os.environ.get("RSSYNC_LIB") or os.path.join(_HERE, "librssync_core.so")


REDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_size_t, C.c_void_p)

_PD = C.POINTER(C.c_double)
_PF = C.POINTER(C.c_float)
_PI64 = C.POINTER(C.c_int64)
_PI32 = C.POINTER(C.c_int32)
_PU64 = C.POINTER(C.c_uint64)

# name -> (restype, argtypes): every symbol include/rssync_c.h declares
SIGNATURES = {
    "rssync_create": (C.c_void_p, []),
    "rssync_ext_borrow": (C.c_void_p, [C.c_void_p]),
    "rssync_destroy": (None, [C.c_void_p]),
    "rssync_last_error": (C.c_char_p, []),
    "rssync_set_panic_mode": (None, [C.c_int]),
    "rssync_set_gyro_quaternions": (C.c_int, [C.c_void_p, _PD, C.c_size_t, C.c_double, C.c_double]),
    "rssync_set_gyro_quaternions_ts": (C.c_int, [C.c_void_p, _PI64, _PD, C.c_size_t]),
    "rssync_set_track_result": (C.c_int, [C.c_void_p, C.c_int64, _PD, _PD, _PD, _PD, C.c_size_t]),
    "rssync_pre_sync": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_double, C.c_double, _PD, _PD]),
    "rssync_sync": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_double, C.c_double, _PD, _PD]),
    "rssync_debug_pre_sync": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_double, _PD, _PD, C.c_int]),
    "rssync_ext_set_seed": (C.c_int, [C.c_void_p, C.c_uint64]),
    "rssync_ext_set_max_outer_iters": (C.c_int, [C.c_void_p, C.c_int]),
    "rssync_ext_set_verbose": (C.c_int, [C.c_void_p, C.c_int]),
    "rssync_ext_set_lbfgs_reeval": (C.c_int, [C.c_void_p, C.c_int]),
    "rssync_ext_lbfgs_best_not_last": (C.c_int, [C.c_void_p, _PU64]),
    "rssync_ext_set_host_loop": (C.c_int, [C.c_void_p, C.c_int]),
    "rssync_ext_set_hook_device_loop": (C.c_int, [C.c_void_p, C.c_int]),
    "rssync_ext_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rssync_ext_set_devices": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "rssync_ext_device_count": (C.c_int, [C.c_void_p]),
    "rssync_ext_set_reduce_hook": (C.c_int, [C.c_void_p, REDUCE_FN, C.c_void_p]),
    "rssync_ext_rccl_preflight": (C.c_int, [C.c_void_p]),
    "rssync_ext_rccl_library": (C.c_char_p, [C.c_void_p]),
    "rssync_ext_rccl_unique_id": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rssync_ext_rccl_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "rssync_ext_rccl_shutdown": (C.c_int, [C.c_void_p]),
    "rssync_ext_set_tracks_hint": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rssync_ext_exchange_stats": (C.c_int, [C.c_void_p, _PU64, _PU64]),
    "rssync_ext_window_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "rssync_ext_set_executor_check": (C.c_int, [C.c_void_p, C.c_int]),
    "rssync_ext_set_executor_check_every": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rssync_ext_executor_stats": (C.c_int, [C.c_void_p, _PU64, _PU64, C.POINTER(C.c_uint32)]),
    "rssync_ext_executor_mismatches": (C.c_int, [C.c_void_p, _PU64]),
    "rssync_ext_near_static_stats": (C.c_int, [C.c_void_p, _PU64, _PU64, _PU64]),
    "rssync_ext_debug_residuals": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32]),
    "rssync_ext_debug_residuals_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32)]),
    "rssync_ext_debug_contenders_get": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]),
    "rssync_ext_record_init_winners": (C.c_int, [C.c_void_p, C.c_int]),
    "rssync_ext_last_init_winners": (C.c_int, [C.c_void_p, _PI32, C.c_size_t, C.POINTER(C.c_size_t)]),
    "rssync_ext_set_init_override": (C.c_int, [C.c_void_p, _PI32, C.c_size_t]),
    "rssync_ext_debug_math64": (C.c_int, [C.c_void_p, C.c_int, _PD, _PD, _PD, C.c_size_t]),
    "rssync_ext_upload": (C.c_int, [C.c_void_p]),
    "rssync_ext_sample_rate": (C.c_int, [C.c_void_p, _PD, _PD, C.POINTER(C.c_size_t)]),
    "rssync_ext_gyro_knots": (C.c_int, [C.c_void_p, _PD, C.c_size_t]),
    "rssync_ext_gyro_table": (C.c_int, [C.c_void_p, _PD, C.c_size_t]),
    "rssync_ext_presync_curve": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_double, C.c_double,
                                           _PD, _PD, C.c_int, C.POINTER(C.c_int), _PD, _PI32, C.POINTER(C.c_int)]),
    "rssync_ext_problem_matrix": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, _PF, _PF, C.c_size_t,
                                            C.POINTER(C.c_size_t)]),
    "rssync_ext_init_motion": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, C.c_int64, _PD, _PD, C.c_int,
                                         C.POINTER(C.c_int)]),
    "rssync_ext_opt_motion": (C.c_int, [C.c_void_p, C.c_double, _PD, _PD, C.c_int, C.POINTER(C.c_int), _PU64, _PU64]),
    "rssync_ext_set_motion": (C.c_int, [C.c_void_p, _PD, _PD, C.c_int]),
    "rssync_ext_loss": (C.c_int, [C.c_void_p, _PD, C.c_int, _PD, _PD]),
    "rssync_ext_sync_simplified": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, C.c_int64, C.c_double, C.c_double, _PD, _PD]),
    "rssync_ext_init_k_simplified": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, C.c_int64, _PD, C.c_int,
                                               C.POINTER(C.c_int)]),
    "rssync_ext_loss_simplified": (C.c_int, [C.c_void_p, _PD, C.c_int, _PD, _PD]),
    "rssync_ext_problem_matrix64": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, _PD, _PD, C.c_size_t,
                                              C.POINTER(C.c_size_t)]),
    "rssync_ext_set_track_pixels": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, _PD, _PD, C.c_size_t,
                                              C.c_void_p, C.c_double]),
    "rssync_ext_set_gyro_rates": (C.c_int, [C.c_void_p, _PD, _PD, C.c_size_t, C.c_char_p]),
    "rssync_ext_set_gyro_conditioning": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rssync_ext_gyro_conditioned": (C.c_int, [C.c_void_p, _PD, C.c_size_t, C.POINTER(C.c_size_t), _PD, _PD]),
    "rssync_ext_orientation_sweep": (C.c_int, [C.c_void_p, _PD, _PD, C.c_size_t, C.POINTER(C.c_char_p), C.c_int,
                                               C.c_double, C.c_int64, C.c_int64, C.c_double, C.c_double, _PD, _PD]),
    "rssync_ext_readout_sweep": (C.c_int, [C.c_void_p, _PD, C.c_int, C.c_double, C.c_int64, C.c_int64, C.c_double,
                                           C.c_double, _PD, _PD]),
    "rssync_ext_set_readout": (C.c_int, [C.c_void_p, C.c_double]),
    "rssync_ext_lens_sweep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int64, C.c_int64, C.c_double,
                                        C.c_double, _PD, _PD]),
    "rssync_ext_set_lens": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rssync_ext_frame_rays": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.POINTER(C.c_size_t)]),
    "rssync_ext_pre_sync_windows": (C.c_int, [C.c_void_p, C.c_double, _PI64, _PI64, C.c_int, C.c_double, C.c_double,
                                              _PD, _PD]),
    "rssync_ext_sync_windows": (C.c_int, [C.c_void_p, _PD, _PI64, _PI64, C.c_int, C.c_double, C.c_double, _PD, _PD]),
    "rssync_ext_sync_points": (C.c_int, [C.c_void_p, _PI64, C.c_int, C.c_int64, C.c_double, C.c_int, C.c_double,
                                         C.c_double, C.c_int, _PD, _PD]),
    "rssync_ext_window_trace": (C.c_int, [C.c_void_p, C.c_int, _PD, C.c_int, C.POINTER(C.c_int)]),
    "rssync_ext_sync_trace": (C.c_int, [C.c_void_p, _PD, C.c_int, C.POINTER(C.c_int)]),
    "rssync_ext_device_context": (C.c_void_p, [C.c_void_p]),
    "rssync_ext_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "rssync_ext_profile_get": (C.c_int, [C.c_void_p, C.c_int, _PU64, _PD]),
    "rssync_ext_profile_reset": (C.c_int, [C.c_void_p]),
}


def bind(lib, signatures=SIGNATURES):
    """Attach a table of C-ABI signatures (include/rssync_c.h's, or a front door's own) to a loaded library."""
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def load_library():
    """dlopen librssync_core.so and bind every C-ABI symbol; raises if it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RsSyncError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C rs-sync_amd/csrc); there is no fallback implementation")
    _LIB = bind(C.CDLL(path))
    return _LIB


_ATTACHED = {}      # id of a front door's signature table -> the library it was attached to


def product_library(signatures):
    """The product library with a front door's signature table attached, once per loaded library (a missing symbol raises)."""
    lib = load_library()
    if _ATTACHED.get(id(signatures)) is not lib:
        bind(lib, signatures)
        _ATTACHED[id(signatures)] = lib
    return lib


def product_only(problem, lib, who):
    """-> lib, the product library, for a call of front door `who` on `problem`: the front doors have no CPU test double."""
    if problem._lib is not lib:
        raise RsSyncError("%s runs in the product library only" % who)
    return lib


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t=_PD):
    return a.ctypes.data_as(t)


class SyncProblem:
    """``CreateSyncProblem()`` + the six ``ISyncProblem`` methods (rssync.h:9-31)."""

    def __init__(self, seed=None, max_outer_iters=None, verbose=False, _lib=None):
        # _lib: tests pass a build of the same host code linked against a CPU test double of the
        # device ABI (tests/cpu_device); the package itself only ever loads librssync_core.so
        self._lib = _lib if _lib is not None else load_library()
        self._lib.rssync_set_panic_mode(1)  # report panics as exceptions instead of exit(1)
        self._h = self._lib.rssync_create()
        if not self._h:
            raise RsSyncError("rssync_create failed: " + self._lib.rssync_last_error().decode())
        self._hook = None
        self._hook_error = None
        self._lib.rssync_ext_set_verbose(self._h, 1 if verbose else 0)
        if seed is not None:
            self._lib.rssync_ext_set_seed(self._h, int(seed))
        if max_outer_iters is not None:
            self._lib.rssync_ext_set_max_outer_iters(self._h, int(max_outer_iters))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rssync_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            err = RsSyncError(self._lib.rssync_last_error().decode())
            cause, self._hook_error = self._hook_error, None
            if cause is not None:
                raise err from cause  # the exception a Python reduce hook raised
            raise err

    # ---- ISyncProblem -------------------------------------------------------
    def SetGyroQuaternions(self, data, sample_rate, first_timestamp):
        """rssync.h:13-14: `data` is (count, 4) [w,x,y,z] at a fixed rate (Hz), first sample time in s."""
        q = _d(data).reshape(-1, 4)
        self._check(self._lib.rssync_set_gyro_quaternions(self._h, _p(q), q.shape[0], float(sample_rate),
                                                          float(first_timestamp)))

    def SetGyroQuaternionsTimestamped(self, timestamps_us, quats):
        """rssync.h:15-16 (the int64-timestamp overload)."""
        ts = np.ascontiguousarray(timestamps_us, dtype=np.int64)
        q = _d(quats).reshape(-1, 4)
        assert ts.shape[0] == q.shape[0]
        self._check(self._lib.rssync_set_gyro_quaternions_ts(self._h, _p(ts, _PI64), _p(q), q.shape[0]))

    def SetTrackResult(self, frame, ts_a, ts_b, rays_a, rays_b):
        """rssync.h:17-18: rays are (count, 3) unit vectors, timestamps in seconds."""
        ta, tb, ra, rb = _d(ts_a), _d(ts_b), _d(rays_a).reshape(-1, 3), _d(rays_b).reshape(-1, 3)
        n = ta.shape[0]
        assert tb.shape[0] == n and ra.shape[0] == n and rb.shape[0] == n
        self._check(self._lib.rssync_set_track_result(self._h, int(frame), _p(ta), _p(tb), _p(ra), _p(rb), n))

    def PreSync(self, initial_delay, frame_begin, frame_end, search_step, search_radius):
        """rssync.h:19-21 -> (cost, delay); frame_end exclusive."""
        c, d = C.c_double(), C.c_double()
        self._check(self._lib.rssync_pre_sync(self._h, initial_delay, frame_begin, frame_end, search_step,
                                              search_radius, C.byref(c), C.byref(d)))
        return c.value, d.value

    def Sync(self, initial_delay, frame_begin, frame_end, search_center, search_radius):
        """rssync.h:22-24 -> (cost, delay); frame_end inclusive."""
        c, d = C.c_double(), C.c_double()
        self._check(self._lib.rssync_sync(self._h, initial_delay, frame_begin, frame_end, search_center,
                                          search_radius, C.byref(c), C.byref(d)))
        return c.value, d.value

    def DebugPreSync(self, initial_delay, frame_begin, frame_end, search_radius, point_count):
        """rssync.h:26-28 -> (delays, costs)."""
        delays = np.zeros(point_count)
        costs = np.zeros(point_count)
        self._check(self._lib.rssync_debug_pre_sync(self._h, initial_delay, frame_begin, frame_end, search_radius,
                                                    _p(delays), _p(costs), point_count))
        return delays, costs

    # ---- extensions (include/rssync_c.h, rssync_ext_*) ----------------------
    def set_seed(self, seed):
        self._lib.rssync_ext_set_seed(self._h, int(seed))

    def set_max_outer_iters(self, n):
        self._lib.rssync_ext_set_max_outer_iters(self._h, int(n))

    def set_lbfgs_reeval(self, reeval):
        """False (default): a line search whose best step is not its last leaves value and gradient as
        the last trial computed them (published ens::L_BFGS); True: re-evaluate at the best step."""
        self._check(self._lib.rssync_ext_set_lbfgs_reeval(self._h, 1 if reeval else 0))

    def set_host_loop(self, host_loop=True):
        """keep Sync's outer loop on the host (it runs on the device where one GPU holds all frames)"""
        self._lib.rssync_ext_set_host_loop(self._h, 1 if host_loop else 0)

    def set_hook_device_loop(self, on=True):
        """with a reduce hook: Sync's loop on the device, the hook called between the kernels on the window sums"""
        self._lib.rssync_ext_set_hook_device_loop(self._h, 1 if on else 0)

    def lbfgs_best_not_last(self):
        n = C.c_uint64()
        self._lib.rssync_ext_lbfgs_best_not_last(self._h, C.byref(n))
        return n.value

    def set_devices(self, device_ids):
        """Spread this object's frames over several GPUs of the process (list of device ordinals)."""
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        self._check(self._lib.rssync_ext_set_devices(self._h, ids, len(device_ids)))

    def device_count(self):
        return int(self._lib.rssync_ext_device_count(self._h))

    def set_stream(self, hip_stream_ptr):
        self._check(self._lib.rssync_ext_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0)))

    def set_reduce_hook(self, fn):
        """fn(np.ndarray float64) must sum the array in place over all ranks; None = single rank."""
        if fn is None:
            self._hook = None
            self._lib.rssync_ext_set_reduce_hook(self._h, C.cast(None, REDUCE_FN), None)
            return

        def tramp(buf, n, _user):
            # ctypes swallows exceptions raised inside a callback: report them as a status instead,
            # which the library turns into a panic (a skipped all-reduce must never go unnoticed)
            try:
                arr = np.ctypeslib.as_array(buf, shape=(n,))
                fn(arr)
                return 0
            except BaseException as exc:  # noqa: BLE001
                self._hook_error = exc
                return 1

        self._hook = REDUCE_FN(tramp)  # keep the trampoline alive
        self._lib.rssync_ext_set_reduce_hook(self._h, self._hook, None)

    def rccl_preflight(self):
        """raises unless this process can use RCCL (library + entry points resolve); no communication"""
        self._check(self._lib.rssync_ext_rccl_preflight(self._h))

    def rccl_library(self):
        return (self._lib.rssync_ext_rccl_library(self._h) or b"").decode()

    def rccl_unique_id(self):
        """128 opaque bytes from ncclGetUniqueId (call on rank 0, hand them to every rank)."""
        buf = C.create_string_buffer(128)
        self._check(self._lib.rssync_ext_rccl_unique_id(self._h, buf))
        return buf.raw

    def rccl_init(self, unique_id, rank, world_size):
        """Join the library's own RCCL communicator; replaces the reduce hook."""
        if len(unique_id) != 128:
            raise ValueError("unique_id must be the 128 bytes of rccl_unique_id()")
        self._check(self._lib.rssync_ext_rccl_init(self._h, C.create_string_buffer(unique_id, 128), int(rank),
                                                   int(world_size)))

    def rccl_shutdown(self):
        """Leave the library's RCCL communicator (collective)."""
        self._check(self._lib.rssync_ext_rccl_shutdown(self._h))

    def set_tracks_hint(self, max_tracks_all_ranks):
        """A no-op since round 5 (kept for callers written against round 4, when the kernel shapes followed the problem's
        largest frame and ranks had to agree on it): a frame's kernels follow its own track count."""
        self._lib.rssync_ext_set_tracks_hint(self._h, int(max_tracks_all_ranks))

    def exchange_stats(self):
        """(calls, doubles) exchanged with other ranks so far, through the hook or the native communicator."""
        a, b = C.c_uint64(), C.c_uint64()
        self._lib.rssync_ext_exchange_stats(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def window_info(self):
        """-> dict: how the kernels' LDS spline windows were laid out for this problem's gyro rate"""
        q = (C.c_uint32 * 8)()
        self._check(self._lib.rssync_ext_window_info(self._h, q))
        return dict(frame_span_knots=q[0], fp64_window_knots=q[1], presync_window_knots=q[2] or 80, presync_window_dynamic=bool(q[2]),
                    presync_chunk=q[3], init_window_knots=q[4] or 80, trial_delays_per_pass=q[5], frame_ends_knots=q[6],
                    fp64_window_compact=bool(q[7]))

    def lmeds_shapes(self):
        """-> list of 6: rows / 256 of the LMedS tile the last PreSync sweep used per size class (include/rssync_hip.h:
        rship_lmeds_shapes; 0 = class absent or not the tile kernel)"""
        q = (C.c_uint32 * 6)()
        fn = self._lib.rship_lmeds_shapes
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]
        self._check(fn(C.c_void_p(self.device_context()), q))
        return list(q)

    def set_executor_check(self, on=True):
        """debug mode: every call the window executor runs is re-run by the launch chain and must give the same bits"""
        self._check(self._lib.rssync_ext_set_executor_check(self._h, 1 if on else 0))

    def set_executor_check_every(self, every):
        """with the check mode off: verify one executor call in `every` against the launch chain (process-wide count; 0 = never)"""
        self._lib.rssync_ext_set_executor_check_every(self._h, int(every))

    def executor_stats(self):
        """-> dict(runs, checked, head, tail, ring_cells, waves) of the window executor on this object"""
        runs, chk, q = C.c_uint64(), C.c_uint64(), (C.c_uint32 * 4)()
        self._check(self._lib.rssync_ext_executor_stats(self._h, C.byref(runs), C.byref(chk), q))
        mm = C.c_uint64()
        self._lib.rssync_ext_executor_mismatches(self._h, C.byref(mm))
        return dict(runs=runs.value, checked=chk.value, head=q[0], tail=q[1], ring_cells=q[2], waves=q[3], mismatches=mm.value)

    def debug_residuals(self, on=True, cap_rows=0):
        """TEST-VARIANTS build only: later sweeps, and later GuessMotion searches (init_motion, Sync), also store the
        |residuals| their LMedS selection worked on"""
        self._check(self._lib.rssync_ext_debug_residuals(self._h, 1 if on else 0, int(cap_rows)))

    def debug_residuals_get(self):
        """-> float32 [candidates][frames][hypotheses][cap_rows] of the last sweep or the last GuessMotion search (one
        candidate, 200 hypotheses), whichever came later (NaN where there is no row)"""
        dims = (C.c_uint32 * 4)()
        self._check(self._lib.rssync_ext_debug_residuals_get(self._h, None, 0, dims))
        out = np.zeros(tuple(int(x) for x in dims), dtype=np.uint32)
        self._check(self._lib.rssync_ext_debug_residuals_get(self._h, _p(out, C.POINTER(C.c_uint32)), out.size, dims))
        return out.view(np.float32)

    def debug_contenders_get(self):
        """TEST-VARIANTS build only, after a GuessMotion search with debug_residuals on -> uint32 [frames]: the contender
        records the tile kernel's search of each frame asked for (more than 24: its record table overflowed)"""
        n = C.c_size_t()
        self._check(self._lib.rssync_ext_debug_contenders_get(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        self._check(self._lib.rssync_ext_debug_contenders_get(self._h, _p(out, C.POINTER(C.c_uint32)), out.size, C.byref(n)))
        return out

    def near_static_stats(self):
        """-> dict(pairs, sweeps): (frame, candidate) pairs of PreSync sweeps recomputed with fp64 rows so far (near-static
        frames, |P| below ~2e-4: core_private.cpp:19-28,45-46 are double), and the sweeps that needed it.  0 on ordinary scenes."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.rssync_ext_near_static_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(pairs=a.value, sweeps=b.value, searches=c.value)

    def record_init_winners(self, on=True):
        self._lib.rssync_ext_record_init_winners(self._h, 1 if on else 0)

    def last_init_winners(self):
        """GuessMotion's winning hypothesis per slot of the last Sync-type call (needs record_init_winners)."""
        n = C.c_size_t()
        self._lib.rssync_ext_last_init_winners(self._h, None, 0, C.byref(n))
        out = np.zeros(n.value, np.int32)
        self._lib.rssync_ext_last_init_winners(self._h, _p(out, _PI32), out.size, C.byref(n))
        return out

    def set_init_override(self, winners):
        """Install these winners instead of the search's in the next Sync-type call (bit-exactness tests)."""
        w = np.ascontiguousarray(winners, np.int32)
        self._lib.rssync_ext_set_init_override(self._h, _p(w, _PI32), w.size)

    def debug_math64(self, op, a, b=None):
        """The Sync kernels' fp64 building blocks on arrays: 0 a/b, 1 sqrt, 2 (log1p, 1/(1+a)), 3 fma(a,b,a), 4 wave sums, 5 a/3 (div3_exact)."""
        a = _d(a)
        b = _d(b) if b is not None else None
        n = a.size
        out = np.zeros(2 * n if op == 2 else ((n + 63) // 64 if op == 4 else n))
        self._check(self._lib.rssync_ext_debug_math64(self._h, int(op), _p(a), _p(b) if b is not None else None, _p(out), n))
        return out.reshape(n, 2) if op == 2 else out

    def upload(self):
        """Pack tracks + spline and copy them to HBM now (otherwise lazy)."""
        self._check(self._lib.rssync_ext_upload(self._h))

    def gyro_info(self):
        fs, st, n = C.c_double(), C.c_double(), C.c_size_t()
        self._lib.rssync_ext_sample_rate(self._h, C.byref(fs), C.byref(st), C.byref(n))
        return fs.value, st.value, n.value

    def gyro_knots(self):
        n = self.gyro_info()[2]
        out = np.zeros((n, 4))
        self._check(self._lib.rssync_ext_gyro_knots(self._h, _p(out), out.size))
        return out

    def gyro_table(self):
        """The device's spline table, (n_knots, 4, 4): [knot][y, b, c, d][w, x, y, z]."""
        n = self.gyro_info()[2]
        out = np.zeros((n, 4, 4))
        self._check(self._lib.rssync_ext_gyro_table(self._h, _p(out), out.size))
        return out

    def presync_curve(self, initial_delay, frame_begin, frame_end, search_step, search_radius, per_frame=False,
                      cap=None):
        if cap is None:
            cap = int(2 * search_radius / search_step) + 8
        delays, costs = np.zeros(cap), np.zeros(cap)
        n, nf = C.c_int(), C.c_int()
        fc = bh = None
        if per_frame:
            if per_frame is True:
                raise ValueError('per_frame must be the number of frames in the range')
            nf_max = int(per_frame)
            fc = np.zeros((cap, nf_max))
            bh = np.zeros((cap, nf_max), dtype=np.int32)
        self._check(self._lib.rssync_ext_presync_curve(
            self._h, initial_delay, frame_begin, frame_end, search_step, search_radius, _p(delays), _p(costs), cap,
            C.byref(n), _p(fc) if per_frame else None, _p(bh, _PI32) if per_frame else None, C.byref(nf)))
        k = n.value
        if per_frame:
            f = nf.value
            fc = fc.reshape(-1)[:k * f].reshape(k, f)
            bh = bh.reshape(-1)[:k * f].reshape(k, f)
            return delays[:k], costs[:k], fc, bh
        return delays[:k], costs[:k]

    def problem_matrix(self, frame, delay, n_tracks, deriv=False):
        P = np.zeros((n_tracks, 3), dtype=np.float32)
        dP = np.zeros((n_tracks, 3), dtype=np.float32) if deriv else None
        n = C.c_size_t()
        self._check(self._lib.rssync_ext_problem_matrix(self._h, int(frame), float(delay), _p(P, _PF),
                                                        _p(dP, _PF) if deriv else None, n_tracks, C.byref(n)))
        return (P[:n.value], dP[:n.value]) if deriv else P[:n.value]

    def problem_matrix64(self, frame, delay, n_tracks, deriv=False):
        """P (and dP/d-delay) as the Sync kernels compute it, fp64"""
        P = np.zeros((n_tracks, 3))
        dP = np.zeros((n_tracks, 3)) if deriv else None
        n = C.c_size_t()
        self._check(self._lib.rssync_ext_problem_matrix64(self._h, int(frame), float(delay), _p(P),
                                                          _p(dP) if deriv else None, n_tracks, C.byref(n)))
        return (P[:n.value], dP[:n.value]) if deriv else P[:n.value]

    def SyncSimplified(self, initial_delay, frame_begin, frame_end, search_center, search_radius):
        """Sync with translation neglected (thesis section 2.11 eq. (12)) -> (cost, delay); frame_end inclusive."""
        c, d = C.c_double(), C.c_double()
        self._check(self._lib.rssync_ext_sync_simplified(self._h, initial_delay, frame_begin, frame_end, search_center,
                                                         search_radius, C.byref(c), C.byref(d)))
        return c.value, d.value

    def init_k_simplified(self, delay, frame_begin, frame_end, cap=1 << 16):
        k, n = np.zeros(cap), C.c_int()
        self._check(self._lib.rssync_ext_init_k_simplified(self._h, delay, frame_begin, frame_end, _p(k), cap, C.byref(n)))
        return k[:n.value].copy()

    def loss_simplified(self, delays, grad=False):
        d = _d(np.atleast_1d(delays))
        out = np.zeros(d.shape[0])
        g = np.zeros(d.shape[0]) if grad else None
        self._check(self._lib.rssync_ext_loss_simplified(self._h, _p(d), d.shape[0], _p(out), _p(g) if grad else None))
        return (out, g) if grad else out

    def init_motion(self, delay, frame_begin, frame_end, cap=1 << 16):
        M, k, n = np.zeros((cap, 3)), np.zeros(cap), C.c_int()
        self._check(self._lib.rssync_ext_init_motion(self._h, delay, frame_begin, frame_end, _p(M), _p(k), cap,
                                                     C.byref(n)))
        return M[:n.value].copy(), k[:n.value].copy()

    def opt_motion(self, delay, cap=1 << 16):
        M, k, n = np.zeros((cap, 3)), np.zeros(cap), C.c_int()
        it, ev = C.c_uint64(), C.c_uint64()
        self._check(self._lib.rssync_ext_opt_motion(self._h, delay, _p(M), _p(k), cap, C.byref(n), C.byref(it),
                                                    C.byref(ev)))
        return M[:n.value].copy(), k[:n.value].copy(), it.value, ev.value

    def set_motion(self, M, k):
        M, k = _d(M).reshape(-1, 3), _d(k)
        self._check(self._lib.rssync_ext_set_motion(self._h, _p(M), _p(k), k.shape[0]))

    def loss(self, delays, grad=False):
        d = _d(np.atleast_1d(delays))
        out = np.zeros(d.shape[0])
        g = np.zeros(d.shape[0]) if grad else None
        self._check(self._lib.rssync_ext_loss(self._h, _p(d), d.shape[0], _p(out), _p(g) if grad else None))
        return (out, g) if grad else out

    def set_track_pixels(self, frame, frame_time_a, frame_time_b, points_a, points_b, lens, image_rows):
        """Tracked pixel positions (n x 2 each) of one frame pair; undistortion, normalisation and
        row times (core_testcode.cpp:135-158) happen on the device.  lens = (ro, fx, fy, cx, cy,
        k1, k2, k3, k4)."""
        a = np.ascontiguousarray(points_a, np.float64)
        b = np.ascontiguousarray(points_b, np.float64)
        if a.ndim != 2 or a.shape[1] != 2 or a.shape != b.shape:
            raise ValueError("points_a / points_b must both be (n, 2)")
        L = np.ascontiguousarray(lens, np.float64)
        if L.shape != (9,):
            raise ValueError("lens = (ro, fx, fy, cx, cy, k1, k2, k3, k4)")
        self._check(self._lib.rssync_ext_set_track_pixels(self._h, int(frame), float(frame_time_a),
                                                          float(frame_time_b), _p(a), _p(b), a.shape[0],
                                                          L.ctypes.data, float(image_rows)))

    def set_gyro_rates(self, timestamps_s, rates, orientation=None):
        """Angular rates (n x 3, rad/s) at timestamps (s): integrated as the reference driver does
        (core_testcode.cpp:36-52) and passed to the timestamped gyro setter."""
        t = np.ascontiguousarray(timestamps_s, np.float64)
        r = np.ascontiguousarray(rates, np.float64)
        if r.ndim != 2 or r.shape[1] != 3 or t.shape != (r.shape[0],):
            raise ValueError("rates must be (n, 3) and timestamps (n,)")
        self._check(self._lib.rssync_ext_set_gyro_rates(self._h, _p(t), _p(r), r.shape[0],
                                                        orientation.encode() if orientation else None))

    def set_gyro_conditioning(self, lowpass_divider=0, decimate=0):
        """What set_gyro_rates / orientation_sweep do with the rates from now on.  ``set_gyro_conditioning(None)``: off
        (every raw sample is integrated).  Otherwise the uniform route on the device: rates -> uniform grid at the rate
        rounded to 50 Hz -> zero-phase Butterworth with cut-off grid rate / lowpass_divider (0: none) -> every
        decimate-th sample (0: all) -> fixed-rate integration.  Recommended for high-rate logs:
        ``lowpass_divider = 4 * decimate``."""
        if lowpass_divider is None:
            self._check(self._lib.rssync_ext_set_gyro_conditioning(self._h, None))
            return
        cfg = (C.c_int32 * 2)(int(lowpass_divider), int(decimate))
        self._check(self._lib.rssync_ext_set_gyro_conditioning(self._h, C.addressof(cfg)))

    def gyro_conditioned(self):
        """What the last set_gyro_rates / orientation_sweep integrated under conditioning, before the orientation is
        applied -> (rates (n, 3), sample rate after decimation, time of sample 0)."""
        n, fs, t0 = C.c_size_t(), C.c_double(), C.c_double()
        self._check(self._lib.rssync_ext_gyro_conditioned(self._h, None, 0, C.byref(n), C.byref(fs), C.byref(t0)))
        out = np.zeros((n.value, 3))
        self._check(self._lib.rssync_ext_gyro_conditioned(self._h, _p(out), n.value, None, None, None))
        return out, fs.value, t0.value

    def orientation_sweep(self, timestamps_s, rates, orientations, initial_delay, frame_begin, frame_end,
                          search_step, search_radius):
        """core_testcode.cpp:186-224: PreSync under every candidate IMU orientation ->
        (costs[n], delays[n]); the true orientation has the lowest cost."""
        t = np.ascontiguousarray(timestamps_s, np.float64)
        r = np.ascontiguousarray(rates, np.float64)
        if r.ndim != 2 or r.shape[1] != 3 or t.shape != (r.shape[0],):
            raise ValueError("rates must be (n, 3) and timestamps (n,)")
        names = (C.c_char_p * len(orientations))(*[o.encode() for o in orientations])
        costs, delays = np.zeros(len(orientations)), np.zeros(len(orientations))
        self._check(self._lib.rssync_ext_orientation_sweep(self._h, _p(t), _p(r), r.shape[0], names,
                                                           len(orientations), float(initial_delay), int(frame_begin),
                                                           int(frame_end), float(search_step), float(search_radius),
                                                           _p(costs), _p(delays)))
        return costs, delays

    def readout_sweep(self, readouts, initial_delay, frame_begin, frame_end, search_step, search_radius):
        """PreSync with every pixel frame of [frame_begin, frame_end) re-timed to each candidate readout (s) ->
        (costs[n], delays[n]); the lowest cost marks the readout that fits.  The frames keep their own readout."""
        ro = np.ascontiguousarray(readouts, np.float64).reshape(-1)
        costs, delays = np.zeros(ro.size), np.zeros(ro.size)
        self._check(self._lib.rssync_ext_readout_sweep(self._h, _p(ro), ro.size, float(initial_delay), int(frame_begin),
                                                       int(frame_end), float(search_step), float(search_radius),
                                                       _p(costs), _p(delays)))
        return costs, delays

    def set_readout(self, ro):
        """Every pixel frame as if set again with lens.ro = ro (s)."""
        self._check(self._lib.rssync_ext_set_readout(self._h, float(ro)))

    def lens_sweep(self, lenses, initial_delay, frame_begin, frame_end, search_step, search_radius):
        """PreSync with every pixel frame of [frame_begin, frame_end) set again with each candidate lens (n x 9, the
        order of set_track_pixels' lens: ro, fx, fy, cx, cy, k1 .. k4) -> (costs[n], delays[n]); the lowest cost marks
        the lens that fits (rssync_amd.lens.estimate_lens searches with it).  The frames keep their own lens."""
        L = np.ascontiguousarray(lenses, np.float64)
        if L.ndim != 2 or L.shape[1] != 9:
            raise ValueError("lenses must be (n, 9): ro, fx, fy, cx, cy, k1, k2, k3, k4 per row")
        n = L.shape[0]
        costs, delays = np.zeros(n), np.zeros(n)
        self._check(self._lib.rssync_ext_lens_sweep(self._h, L.ctypes.data, n, float(initial_delay), int(frame_begin),
                                                    int(frame_end), float(search_step), float(search_radius),
                                                    _p(costs), _p(delays)))
        return costs, delays

    def set_lens(self, lens):
        """Every pixel frame as if set again with this lens (ro, fx, fy, cx, cy, k1, k2, k3, k4)."""
        L = np.ascontiguousarray(lens, np.float64)
        if L.shape != (9,):
            raise ValueError("lens = (ro, fx, fy, cx, cy, k1, k2, k3, k4)")
        self._check(self._lib.rssync_ext_set_lens(self._h, L.ctypes.data))

    def frame_rays(self, frame, cap=2048):
        """The packed device streams of one frame: ({ax,bx,ay,by}, {az,bz,ta,tb}) as (n, 4) float32."""
        a4, b4, n = np.zeros((cap, 4), np.float32), np.zeros((cap, 4), np.float32), C.c_size_t()
        self._check(self._lib.rssync_ext_frame_rays(self._h, int(frame), a4.ctypes.data, b4.ctypes.data, cap,
                                                    C.byref(n)))
        return a4[:n.value].copy(), b4[:n.value].copy()

    def pre_sync_windows(self, initial_delay, frame_begins, frame_ends, search_step, search_radius):
        """PreSync on W windows [begin[w], end[w]) in one sweep -> (costs[W], delays[W])."""
        b = np.ascontiguousarray(frame_begins, np.int64)
        e = np.ascontiguousarray(frame_ends, np.int64)
        if b.shape != e.shape or b.ndim != 1:
            raise ValueError("frame_begins / frame_ends must be 1-D and of equal length")
        costs, delays = np.zeros(b.size), np.zeros(b.size)
        self._check(self._lib.rssync_ext_pre_sync_windows(self._h, float(initial_delay), _p(b, _PI64), _p(e, _PI64), b.size,
                                                          float(search_step), float(search_radius), _p(costs),
                                                          _p(delays)))
        return costs, delays

    def sync_windows(self, initial_delays, frame_begins, frame_ends, search_center, search_radius):
        """Sync on W windows [begin[w], end[w]] advanced in lock-step -> (costs[W], delays[W])."""
        b = np.ascontiguousarray(frame_begins, np.int64)
        e = np.ascontiguousarray(frame_ends, np.int64)
        d0 = np.ascontiguousarray(np.broadcast_to(np.asarray(initial_delays, np.float64), b.shape))
        if b.shape != e.shape or b.ndim != 1:
            raise ValueError("frame_begins / frame_ends must be 1-D and of equal length")
        costs, delays = np.zeros(b.size), np.zeros(b.size)
        self._check(self._lib.rssync_ext_sync_windows(self._h, _p(d0), _p(b, _PI64), _p(e, _PI64), b.size,
                                                      float(search_center), float(search_radius), _p(costs),
                                                      _p(delays)))
        return costs, delays

    def sync_points(self, positions, sync_window, initial_delay, presync_step=None, presync_radius=None, repeats=4):
        """The reference driver's loop (core_testcode.cpp:303-316) over all sync points at once:
        optional PreSync, then `repeats` chained Sync calls per position -> (costs[W], delays[W])."""
        pos = np.ascontiguousarray(positions, np.int64)
        if pos.ndim != 1:
            raise ValueError("positions must be 1-D")
        use = presync_step is not None and presync_radius is not None
        costs, delays = np.zeros(pos.size), np.zeros(pos.size)
        self._check(self._lib.rssync_ext_sync_points(self._h, _p(pos, _PI64), pos.size, int(sync_window),
                                                     float(initial_delay), 1 if use else 0,
                                                     float(presync_step) if use else 0.0,
                                                     float(presync_radius) if use else 0.0, int(repeats), _p(costs),
                                                     _p(delays)))
        return costs, delays

    def window_trace(self, window, cap=2048):
        t, n = np.zeros((cap, 6)), C.c_int()
        self._check(self._lib.rssync_ext_window_trace(self._h, int(window), _p(t), cap, C.byref(n)))
        return t[:min(n.value, cap)].copy()

    def sync_trace(self, cap=512):
        t, n = np.zeros((cap, 6)), C.c_int()
        self._lib.rssync_ext_sync_trace(self._h, _p(t), cap, C.byref(n))
        return t[:min(n.value, cap)].copy()

    def track_points(self, frames, grid_step=200, **params):
        """Sparse pyramidal Lucas-Kanade at the driver's grid (include/rssync_track.h, rssync_amd.track): frames is an
        (n, H, W) uint8 numpy array or a uint8 torch tensor on this problem's device ->
        (points_a (P, 2), points_b (n-1, P, 2), status (n-1, P) uint8, residual (n-1, P) float32).  params: window,
        levels, max_iters, epsilon, min_eig.  Nothing is stored in the problem."""
        from . import track
        return track.track_points(self, frames, grid_step=grid_step, **params)

    def track_frames(self, frames, frame_times, lens, first_frame=0, grid_step=200, **params):
        """track_points, then set_track_pixels(first_frame + k, frame_times[k], frame_times[k+1], grid, b_k, lens, H)
        for every pair k (core_testcode.cpp:97-158).  A long video goes in overlapping batches: INTEGRATION.md."""
        from . import track
        track.track_frames(self, frames, frame_times, lens, first_frame=first_frame, grid_step=grid_step, **params)

    def track_features(self, frames, **params):
        """Corner features per cell, tracked forward and backward (include/rssync_features.h, rssync_amd.features):
        frames as in track_points -> Features(counts, points_a, points_b, status, fb_error), one row per pair whose
        first counts[k] entries are set.  params: cell, block, quality, max_fb_error and the LK settings of
        track_points.  Nothing is stored in the problem."""
        from . import features
        return features.track_features(self, frames, **params)

    def features_frames(self, frames, frame_times, lens, first_frame=0, **params):
        """track_features, then set_track_pixels(first_frame + k, frame_times[k], frame_times[k+1], a_k, b_k, lens, H)
        with the status-0 tracks of every pair keeping at least min_tracks (default 8) -> the pairs handed on."""
        from . import features
        return features.features_frames(self, frames, frame_times, lens, first_frame=first_frame, **params)

    def rectify_frames(self, frames, frame_times, lens, delay, **params):
        """The frames with the rolling-shutter skew removed (include/rssync_rectify.h, rssync_amd.rectify): what a
        global-shutter camera with the same lens would have seen at the orientation of ref_row's time, from the installed
        gyro data and `delay`.  frames as in track_points -> (frames of the same kind, n_outside (n,)).  params: ref_row,
        iterations, fill, out."""
        from . import rectify
        return rectify.rectify_frames(self, frames, frame_times, lens, delay, **params)

    def rectify_map(self, width, height, lens, frame_time, delay, **params):
        """-> (H, W, 2) float32: where rectify_frames looks every output pixel up.  params: ref_row, iterations."""
        from . import rectify
        return rectify.rectify_map(self, width, height, lens, frame_time, delay, **params)

    def rectify_points(self, points, width, height, lens, frame_time, delay, ref_row=None):
        """Tracked points (..., 2) of a rolling-shutter frame -> their positions in the rectified frame (float64)."""
        from . import rectify
        return rectify.rectify_points(self, points, width, height, lens, frame_time, delay, ref_row=ref_row)

    def stabilize_path(self, frame_times, ro, delay, sigma, out=None):
        """-> (n, 4) float64: the Gaussian-smoothed orientation (w, x, y, z) at every frame's centre time
        (include/rssync_stabilize.h, rssync_amd.stabilize)."""
        from . import stabilize
        return stabilize.stabilize_path(self, frame_times, ro, delay, sigma, out=out)

    def stabilize_map(self, width, height, lens, frame_time, delay, **params):
        """-> (out_height, out_width, 2) float32: where stabilize_frames looks every output pixel up.  params: target,
        out_size, sigma, zoom, camera, out_camera, iterations."""
        from . import stabilize
        return stabilize.stabilize_map(self, width, height, lens, frame_time, delay, **params)

    def stabilize_frames(self, frames, frame_times, lens, delay, **params):
        """The frames rendered at the smoothed path's orientations, or at `targets` -> (frames of the same kind,
        n_outside (n,)).  params: targets, out_size, out, sigma, zoom, camera, out_camera, iterations, fill, filter
        (stabilize.FILTER_BILINEAR, the default, or FILTER_BICUBIC)."""
        from . import stabilize
        return stabilize.stabilize_frames(self, frames, frame_times, lens, delay, **params)

    def stabilize_coverage(self, width, height, lens, frame_times, delay, zooms, **params):
        """-> (n_frames, n_zooms) uint32: output border pixels that see past the frame, per frame and zoom."""
        from . import stabilize
        return stabilize.stabilize_coverage(self, width, height, lens, frame_times, delay, zooms, **params)

    def stabilize_zoom(self, width, height, lens, frame_times, delay, zooms, **params):
        """-> the smallest zoom of `zooms` that keeps the borders out of every frame, or None."""
        from . import stabilize
        return stabilize.stabilize_zoom(self, width, height, lens, frame_times, delay, zooms, **params)

    def fit_zoom(self, width, height, lens, frame_times, delay, lo, hi, **params):
        """-> (zooms (n,), status (n,)): every frame's smallest zoom in [lo, hi] that keeps the output's borders inside the
        frame, found by a bisection on the device (include/rssync_zoom.h, rssync_amd.zoom).  params: steps, targets,
        out_size, sigma, camera, out_camera, iterations."""
        from . import zoom
        return zoom.fit_zoom(self, width, height, lens, frame_times, delay, lo, hi, **params)

    def smooth_zooms(self, frame_times, zooms, window):
        """-> (n,): the envelope of a fitted zoom curve over `window` seconds, never below the curve."""
        from . import zoom
        return zoom.smooth_zooms(self, frame_times, zooms, window)

    def dynamic_zoom(self, width, height, lens, frame_times, delay, lo, hi, window, **params):
        """-> (n,): fit_zoom followed by smooth_zooms; raises where a frame is not clear at `hi`."""
        from . import zoom
        return zoom.dynamic_zoom(self, width, height, lens, frame_times, delay, lo, hi, window, **params)

    def stabilize_frames_zoomed(self, frames, frame_times, lens, delay, zooms, **params):
        """stabilize_frames with one zoom per frame -> (frames (n, out_height, out_width), n_outside (n,)).  params:
        targets, out_size, out, sigma, camera, out_camera, iterations, fill, filter."""
        from . import zoom
        return zoom.stabilize_frames_zoomed(self, frames, frame_times, lens, delay, zooms, **params)

    def stabilize_frames_zoomed_budget(self, frames, frame_times, lens, delay, zooms, budget_bytes, **params):
        """stabilize_frames_zoomed through the internal launcher with a device budget for its chunk slots (tests)."""
        from . import zoom
        return zoom.stabilize_frames_zoomed_budget(self, frames, frame_times, lens, delay, zooms, budget_bytes, **params)

    def stabilize_frames_infilled(self, frames, frame_times, lens, delay, radius, **params):
        """stabilize_frames with the borders taken from up to `radius` neighbouring frames of the call on each side
        (include/rssync_infill.h, rssync_amd.infill) -> (frames (n, out_height, out_width), n_outside (n,), n_borrowed (n,)).
        params: targets, out_size, out, sigma, zoom, camera, out_camera, iterations, fill, filter."""
        from . import infill
        return infill.stabilize_frames_infilled(self, frames, frame_times, lens, delay, radius, **params)

    def stabilize_frames_infilled_budget(self, frames, frame_times, lens, delay, radius, budget_bytes, **params):
        """stabilize_frames_infilled through the internal launcher with a device budget for its chunk slots (tests)."""
        from . import infill
        return infill.stabilize_frames_infilled_budget(self, frames, frame_times, lens, delay, radius, budget_bytes, **params)

    def stabilize_color_infilled(self, fmt, frames, frame_times, lens, delay, radius, **params):
        """stabilize_color with the borders of every plane taken from up to `radius` neighbouring frames of the call on each
        side (include/rssync_colorinfill.h, rssync_amd.colorinfill) -> (frames in the layout of `frames`, n_outside (n, 2),
        n_borrowed (n, 2)).  params: targets, out_size, out, n_borrowed, chroma_site, fills, sigma, zoom, camera, out_camera,
        iterations, fill, filter."""
        from . import colorinfill
        return colorinfill.stabilize_color_infilled(self, fmt, frames, frame_times, lens, delay, radius, **params)

    def stabilize_color_infilled_budget(self, fmt, frames, frame_times, lens, delay, radius, budget_bytes, **params):
        """stabilize_color_infilled through the internal launcher with a device budget for its chunk slots (tests)."""
        from . import colorinfill
        return colorinfill.stabilize_color_infilled_budget(self, fmt, frames, frame_times, lens, delay, radius, budget_bytes, **params)

    def stabilize_color(self, fmt, frames, frame_times, lens, delay, **params):
        """Colour frames (rssync_amd.color: GRAY8, NV12, I420, RGBA32, and with uint16 samples GRAY16, P010, P016, I010)
        rendered at the smoothed path's orientations, or at `targets`, all planes of a frame in one pass
        (include/rssync_color.h, include/rssync_color16.h) -> (frames in the layout of `frames`,
        n_outside (n, 2)).  params: targets, out_size, out, chroma_site, fills, sigma, zoom, camera, out_camera,
        iterations, fill, filter."""
        from . import color
        return color.stabilize_color(self, fmt, frames, frame_times, lens, delay, **params)

    def color_map(self, fmt, plane, width, height, lens, frame_time, delay, **params):
        """-> float32 (rows, cols, 2): where stabilize_color looks every output sample of `plane` up (plane 1: the chroma
        plane of NV12 and I420, in its own coordinates).  params: target, out_size, chroma_site, sigma, zoom, camera,
        out_camera, iterations."""
        from . import color
        return color.color_map(self, fmt, plane, width, height, lens, frame_time, delay, **params)

    def stabilize_yuv(self, fmt, frames, frame_times, lens, delay, **params):
        """4:2:2 and 4:4:4 frames (rssync_amd.yuv: I422, NV16, I444, and with uint16 samples I210, P210, P216, I410) rendered
        at the smoothed path's orientations, or at `targets`, all planes of a frame in one pass (include/rssync_yuv.h)
        -> (planes in the layout of `frames`, a tuple of arrays or device tensors, n_outside (n, 2)).  params: targets,
        out_size, out, chroma_site, fills, sigma, zoom, camera, out_camera, iterations, fill, filter."""
        from . import yuv
        return yuv.stabilize_yuv(self, fmt, frames, frame_times, lens, delay, **params)

    def stabilize_yuv_budget(self, fmt, frames, frame_times, lens, delay, budget_bytes, **params):
        """stabilize_yuv through the internal launcher with a device budget for its chunk slots (tests)."""
        from . import yuv
        return yuv.stabilize_yuv_budget(self, fmt, frames, frame_times, lens, delay, budget_bytes, **params)

    def yuv_map(self, fmt, plane, width, height, lens, frame_time, delay, **params):
        """-> float32 (rows, cols, 2): where stabilize_yuv looks every output sample of `plane` up (plane 1 of a 4:2:2
        format: the chroma plane, out_width / 2 wide, in its own coordinates; of a 4:4:4 format: plane 0).  params: target,
        out_size, chroma_site, sigma, zoom, camera, out_camera, iterations."""
        from . import yuv
        return yuv.yuv_map(self, fmt, plane, width, height, lens, frame_time, delay, **params)

    def stabilize_color_zoomed(self, fmt, frames, frame_times, lens, delay, zooms, **params):
        """stabilize_color with one zoom per frame (include/rssync_colorzoom.h, rssync_amd.colorzoom) -> (frames in the layout
        of `frames`, n_outside (n, 2)).  params: targets, out_size, out, chroma_site, fills, sigma, camera, out_camera,
        iterations, fill, filter."""
        from . import colorzoom
        return colorzoom.stabilize_color_zoomed(self, fmt, frames, frame_times, lens, delay, zooms, **params)

    def stabilize_color_zoomed_budget(self, fmt, frames, frame_times, lens, delay, zooms, budget_bytes, **params):
        """stabilize_color_zoomed through the internal launcher with a device budget for its chunk slots (tests)."""
        from . import colorzoom
        return colorzoom.stabilize_color_zoomed_budget(self, fmt, frames, frame_times, lens, delay, zooms, budget_bytes, **params)

    def fit_zoom_color(self, fmt, width, height, lens, frame_times, delay, lo, hi, **params):
        """-> (zooms (n,), status (n,)): every frame's smallest zoom in [lo, hi] that clears every plane of the format, a
        4:2:0 chroma plane included.  params: steps, targets, out_size, chroma_site, sigma, camera, out_camera, iterations."""
        from . import colorzoom
        return colorzoom.fit_zoom_color(self, fmt, width, height, lens, frame_times, delay, lo, hi, **params)

    def dynamic_zoom_color(self, fmt, width, height, lens, frame_times, delay, lo, hi, window, **params):
        """-> (n,): fit_zoom_color followed by smooth_zooms; raises where a frame is not clear at `hi`."""
        from . import colorzoom
        return colorzoom.dynamic_zoom_color(self, fmt, width, height, lens, frame_times, delay, lo, hi, window, **params)

    def stabilize_yuv_infilled(self, fmt, frames, frame_times, lens, delay, radius, **params):
        """stabilize_yuv with the borders of every plane taken from up to `radius` neighbouring frames of the call on each
        side (include/rssync_infillyuv.h, rssync_amd.infillyuv) -> (planes in the layout of `frames`, n_outside (n, 2),
        n_borrowed (n, 2)).  params: targets, out_size, out, n_borrowed, chroma_site, fills, sigma, zoom, camera, out_camera,
        iterations, fill, filter."""
        from . import infillyuv
        return infillyuv.stabilize_yuv_infilled(self, fmt, frames, frame_times, lens, delay, radius, **params)

    def stabilize_yuv_infilled_budget(self, fmt, frames, frame_times, lens, delay, radius, budget_bytes, **params):
        """stabilize_yuv_infilled through the internal launcher with a device budget for its chunk slots (tests)."""
        from . import infillyuv
        return infillyuv.stabilize_yuv_infilled_budget(self, fmt, frames, frame_times, lens, delay, radius, budget_bytes, **params)

    def stabilize_yuv_zoomed(self, fmt, frames, frame_times, lens, delay, zooms, **params):
        """stabilize_yuv with one zoom per frame (include/rssync_zoomyuv.h, rssync_amd.zoomyuv) -> (planes in the layout of
        `frames`, n_outside (n, 2)).  params: targets, out_size, out, chroma_site, fills, sigma, camera, out_camera,
        iterations, fill, filter."""
        from . import zoomyuv
        return zoomyuv.stabilize_yuv_zoomed(self, fmt, frames, frame_times, lens, delay, zooms, **params)

    def stabilize_yuv_zoomed_budget(self, fmt, frames, frame_times, lens, delay, zooms, budget_bytes, **params):
        """stabilize_yuv_zoomed through the internal launcher with a device budget for its chunk slots (tests)."""
        from . import zoomyuv
        return zoomyuv.stabilize_yuv_zoomed_budget(self, fmt, frames, frame_times, lens, delay, zooms, budget_bytes, **params)

    def fit_zoom_yuv(self, fmt, width, height, lens, frame_times, delay, lo, hi, **params):
        """-> (zooms (n,), status (n,)): every frame's smallest zoom in [lo, hi] that clears every plane of the format, a
        4:2:2 chroma plane included.  params: steps, targets, out_size, chroma_site, sigma, camera, out_camera, iterations."""
        from . import zoomyuv
        return zoomyuv.fit_zoom_yuv(self, fmt, width, height, lens, frame_times, delay, lo, hi, **params)

    def dynamic_zoom_yuv(self, fmt, width, height, lens, frame_times, delay, lo, hi, window, **params):
        """-> (n,): fit_zoom_yuv followed by smooth_zooms; raises where a frame is not clear at `hi`."""
        from . import zoomyuv
        return zoomyuv.dynamic_zoom_yuv(self, fmt, width, height, lens, frame_times, delay, lo, hi, window, **params)

    def fit_strength(self, width, height, lens, frame_times, delay, **params):
        """-> (strengths (n,), status (n,)): how far every frame may follow its goal at a fixed zoom without showing a
        border, found by a bisection on the device (include/rssync_limit.h, rssync_amd.limit).  params: zoom, zooms, steps,
        targets, out_size, sigma, camera, out_camera, iterations."""
        from . import limit
        return limit.fit_strength(self, width, height, lens, frame_times, delay, **params)

    def smooth_strengths(self, frame_times, strengths, window):
        """-> (n,): the lower envelope of a fitted strength curve over `window` seconds, never above the curve."""
        from . import limit
        return limit.smooth_strengths(self, frame_times, strengths, window)

    def strength_targets(self, frame_times, ro, delay, strengths, **params):
        """-> (n, 4): every frame's target at its strength between its own orientation and its goal.  params: targets, sigma."""
        from . import limit
        return limit.strength_targets(self, frame_times, ro, delay, strengths, **params)

    def limited_targets(self, width, height, lens, frame_times, delay, window, **params):
        """-> (targets (n, 4), strengths (n,), status (n,)): fit_strength, smooth_strengths and the targets that result,
        for any renderer's `targets`.  params: fit_strength's, and verify (one coverage call; raises where not clear)."""
        from . import limit
        return limit.limited_targets(self, width, height, lens, frame_times, delay, window, **params)

    def device_context(self):
        """rship_ctx* of this problem (include/rssync_hip.h), for kernel-level tools."""
        return self._lib.rssync_ext_device_context(self._h)

    def profile(self, enable=True):
        self._check(self._lib.rssync_ext_profile(self._h, 1 if enable else 0))

    def profile_reset(self):
        self._check(self._lib.rssync_ext_profile_reset(self._h))

    def profile_get(self):
        names = ["lmeds", "loss", "motion", "reduce", "init", "pixels", "gyro", "loss_grad", "retime", "relens"]
        out = {}
        for i, nm in enumerate(names):
            n, ms = C.c_uint64(), C.c_double()
            self._check(self._lib.rssync_ext_profile_get(self._h, i, C.byref(n), C.byref(ms)))
            out[nm] = (n.value, ms.value)
        return out
