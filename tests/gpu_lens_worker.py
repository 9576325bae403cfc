"""One rank of the 2-rank lens-sweep test (tests/test_gpu_lens_sweep.py::test_two_ranks_one_exchange_per_sweep): both ranks
share the box's one GPU, gloo carries the sums; rank 0 holds the first half of the pixel frames, rank 1 the rest."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = 24
ARGS = (0.0, 0, F, 0.004, 0.08)


def lenses():
    """six lenses around synth.LENS: focal length, k1, cx and ro moved"""
    from rssync_amd import synth
    ro, fx, fy, cx, cy, k1, k2, k3, k4 = synth.LENS
    return [(ro, 0.9 * fx, 0.9 * fy, cx, cy, k1, k2, k3, k4), tuple(synth.LENS), (ro, 1.1 * fx, 1.1 * fy, cx, cy, k1, k2, k3, k4),
            (ro, fx, fy, cx, cy, k1 - 0.05, k2, k3, k4), (ro, fx, fy, cx + 60.0, cy, k1 + 0.05, k2, k3, k4),
            (0.006, fx, fy, cx, cy, k1, k2, k3, k4)]


def scene():
    from rssync_amd import synth
    gyro = synth.make_gyro(0.0, (F + 2) / synth.FPS, seed=12)
    return gyro, list(synth.make_pixel_frames(gyro, 0, F, 160, seed=12))


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    import rssync_amd
    from rssync_amd import synth
    from rssync_amd.dist import make_reduce_hook
    gyro, frames = scene()
    b, e = (0, F // 2) if rank == 0 else (F // 2, F)
    p = rssync_amd.SyncProblem(seed=321)
    p.SetGyroQuaternions(gyro.quats, gyro.fs, gyro.t0)
    for fr, ta, tb, pa, pb in frames[b:e]:
        p.set_track_pixels(fr, ta, tb, pa, pb, synth.LENS, synth.IMAGE_ROWS)
    p.set_reduce_hook(make_reduce_hook("cpu"))
    p.upload()
    calls0 = p.exchange_stats()[0]
    costs, delays = p.lens_sweep(lenses(), *ARGS)
    calls = p.exchange_stats()[0] - calls0
    with open(out, "w") as f:
        json.dump(dict(rank=rank, costs=costs.tolist(), delays=delays.tolist(), exchanges=calls), f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
