"""Ranked runs for the tests: a reduce hook that checks, before every all-reduce, that every rank exchanges the same number
of doubles, and a launcher of rank workers that kills them all at the first failure or at the timeout.

Every rank must make the same exchanges, in the same order and with the same sizes, whichever frames it holds.  A rank
whose exchange differs would leave the others waiting (gloo: an error or a hang; RCCL: a collective that never completes on
the device); the checking hook turns that into the same error on every rank instead, with every rank's length in it."""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np


class ExchangeMismatch(RuntimeError):
    pass


def checked_reduce_hook():
    """fn(np.ndarray float64) that sums the array in place over all ranks (gloo), after an all-gather of its length; if the
    lengths differ it raises ExchangeMismatch on every rank.  fn.lengths: this rank's lengths, in order."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size()
    lengths = []

    def hook(arr):
        n = int(arr.shape[0])
        lengths.append(n)
        got = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
        dist.all_gather(got, torch.tensor([n], dtype=torch.int64))
        every = [int(t.item()) for t in got]
        if any(m != n for m in every):
            raise ExchangeMismatch("exchange %d: the ranks' lengths differ: %s" % (len(lengths), every))
        t = torch.from_numpy(arr) if arr.flags["C_CONTIGUOUS"] and arr.flags["WRITEABLE"] else None
        if t is not None:
            dist.all_reduce(t)  # in place, on the caller's memory
        else:
            t = torch.tensor(arr, dtype=torch.float64)
            dist.all_reduce(t)
            arr[:] = t.numpy()

    hook.lengths = lengths
    return hook


def bits(values):
    """the exact bits of a float or a sequence of floats, as a list of ints (equal bits <=> equal lists)"""
    return np.atleast_1d(np.asarray(values, np.float64)).view(np.uint64).tolist()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(script, world, args, out_dir, timeout=300, env=None):
    """Start `world` workers `python script rank world port out.json *args`, wait for all of them and return their JSON
    results in rank order.  The first worker that fails, or the timeout, kills every worker and fails the caller (the
    others may be waiting in a collective that will never complete); there is no retry."""
    port = _free_port()
    outs = [os.path.join(str(out_dir), "rank%d.json" % r) for r in range(world)]
    logs = [open(os.path.join(str(out_dir), "rank%d.log" % r), "w+") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, script, str(r), str(world), str(port), outs[r]] + [str(a) for a in args],
                              stdout=logs[r], stderr=subprocess.STDOUT, env=env) for r in range(world)]

    def tail(r):
        logs[r].flush()
        logs[r].seek(0)
        return logs[r].read()[-3000:]

    try:
        deadline = time.monotonic() + timeout
        while True:
            codes = [p.poll() for p in procs]
            bad = [r for r, c in enumerate(codes) if c not in (None, 0)]
            if bad:
                raise AssertionError("rank %d of %d exited with %d:\n%s" % (bad[0], world, codes[bad[0]], tail(bad[0])))
            if all(c == 0 for c in codes):
                break
            if time.monotonic() > deadline:
                late = [r for r, c in enumerate(codes) if c is None]
                raise AssertionError("ranks %s of %d still running after %d s:\n%s" % (late, world, timeout, tail(late[0])))
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
        for f in logs:
            f.close()
    res = []
    for o in outs:
        with open(o) as f:
            res.append(json.load(f))
    return res
