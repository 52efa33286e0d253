"""ctypes binding of the host-side helpers in `include/trs_host.h` (library: `libtrs_host.so`, in-tree; plain C +
OpenMP, no GPU), and the thread budget of their OpenMP teams.

There is no fallback: if the library is missing, `load()` raises `HipExtensionError`.
"""
import ctypes
import os

from .utils import HipExtensionError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtrs_host.so")

_P = ctypes.c_void_p
_I = ctypes.c_int
_D = ctypes.c_double

#: every symbol `include/trs_host.h` declares -> (restype, argtypes)
SIGNATURES = {
    "trs_cubegen_bounds": (_I, [_I, _I, _I, _I, _I, _P, _P]),
    "trs_cubegen": (_I, [_I, ctypes.c_uint64, _I, _I, _I, _P, _I, _I, _I, _D, _D, _P, _I, _I, _P, _I, _I, _I,
                         _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_int64]),
    "trs_ga_update_pop": (_I, [_P, _I, _I, _I, _I, _D, _D, _D, _P, _P, _P, _P]),
    "trs_host_threads": (_I, [_I]),
    "trs_rcm_order": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "trs_profile_order": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I]),
    "trs_envelope_reach": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "trs_apply_joint_order": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "trs_graph_features": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _D, _D, _D, _D, _I,
                                _P, _P, _P, _P, _P]),
    "trs_json_pack": (_I, [_I, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "trs_json_read_files": (_I, [_I, _P, _P, _P]),
    "trs_json_free_files": (None, [_I, _P]),
}

_lib = None


def available_cpus():
    """CPUs this process may actually use: the affinity mask, cut down to the cgroup CPU quota (v2
    `cpu.max`, v1 `cpu.cfs_quota_us`) when the container has one."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, period = fh.read().split()[:2]
            if q != "max":
                quota = int(q) / int(period)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as fq, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fp:
                q, period = int(fq.read()), int(fp.read())
                if q > 0 and period > 0:
                    quota = q / period
        except (OSError, ValueError):
            pass
    if quota is not None:
        n = min(n, max(1, int(quota + 0.5)))
    return max(1, n)


_thread_share = None   # number of processes that share this host's CPUs with this one (set_host_thread_share)


def host_thread_budget(sharers=None):
    """Threads the native host helpers of THIS process may use: the CPUs the container really has
    (`available_cpus`) divided by the number of processes that work side by side on this host - the ranks of a
    `torchrun` launch (`LOCAL_WORLD_SIZE`) or the workers of a `shard.ShardedSolver`.  Eight ranks that each
    start a team of every CPU oversubscribe the host eight times exactly where the ragged workloads are
    host-bound (the joint order, the generator)."""
    if sharers is None:
        sharers = _thread_share
    if sharers is None:
        try:
            sharers = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
        except ValueError:
            sharers = 1
    return max(1, available_cpus() // max(1, int(sharers)))


def set_host_thread_share(sharers):
    """Declare that `sharers` processes share this host (a rank of an N-process job, a worker of a pool of
    N): the OpenMP teams of the native helpers are sized to `host_thread_budget()` from now on
    (`OMP_NUM_THREADS` in the environment still wins).  Returns the budget."""
    global _thread_share
    _thread_share = max(1, int(sharers))
    if _lib is not None and "OMP_NUM_THREADS" not in os.environ:
        _lib.trs_host_threads(host_thread_budget())
    return host_thread_budget()


def host_threads():
    """Size of the OpenMP team the native helpers use right now."""
    return int(load().trs_host_threads(0))


def load():
    """Load the library once, attach the prototypes and size its OpenMP team."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipExtensionError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        if "OMP_NUM_THREADS" not in os.environ:   # a team of every logical CPU is throttled under a CPU quota
            lib.trs_host_threads(host_thread_budget())
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc})")


def ptr(a):
    """The data pointer of a numpy array (which the caller keeps alive over the call), or NULL for None."""
    return None if a is None else a.ctypes.data_as(_P)
