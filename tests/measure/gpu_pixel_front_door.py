"""The pixel front door on the device against the oracle, per lens (tests/test_pixel_front_door.py's checks, measured):
the share of in-image fp32 stream components that differ in any bit from the oracle-fed route, the largest fp32 and
problem_matrix64 differences, and the non-finite counter's K on one context and on two.  GPU box:
`python tests/measure/gpu_pixel_front_door.py [out.json]` (default profiles/pixel_front_door.json)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402,F401  (before the library: torch ships its own HIP runtime)
import rssync_amd  # noqa: E402
import pixel_cases as pc  # noqa: E402


def make(**kw):
    return rssync_amd.SyncProblem(seed=pc.SEED, **kw)


res = {"what": "pack_frames_kernel's pixel branch against the oracle fed the driver's way; point sets of tests/pixel_cases.py",
       "bounds_asserted": {"fp32_component": pc.RAY_TOL32, "in_image_share": 0.01, "p64": pc.P_TOL64},
       "lenses": {}}
for name in pc.LENSES:
    res["lenses"][name] = pc.check_lens(make, name, seed=11).as_dict()
res["counter"] = {"K_expected": pc.COUNTER_K, "K_one_context": pc.check_counter(make),
                  "K_two_contexts": pc.check_counter(make, contexts=2)}
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pixel_front_door.json")
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))
