"""The headline's launch in small, for a profiler to wrap: eight resident 1080p pairs at cfg-2, 5000 features each, STEPS (default 4)
steps of build + batched tracker; prints a hash of every step's records.  Environment: LAZY = KLT_OPT_L0_LAZY_GRAD (0: the records
kernel, 1: the lazy one from the second step on), FORM = KLT_OPT_TRACK_LAZY_FORM (unset: the library's default -- or a library from
before the option, through KLT_GPU_LIB).

    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/lazy_prof/kt_f1 -o run -- python3 tools/lazy_entry_probe.py
    rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES --output-format csv -d /tmp/lazy_prof/pmc_f1_1 -o run -- python3 tools/lazy_entry_probe.py
    python3 tools/lazy_entry_counters.py /tmp/lazy_prof          # durations and counters per launch of the tracker kernels, medians"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyfeaturetrack_amd.params import params_from_tc    # noqa: E402
from benchlib.common import NFEAT, cfg2_context         # noqa: E402
from pyfeaturetrack_amd import synth                    # noqa: E402
from pyfeaturetrack_amd.backend import Context          # noqa: E402

B = 8
STEPS = int(os.environ.get("STEPS", "4"))
pairs = [synth.synth_pair(1920, 1080, seed=s + 1) for s in range(B)]
slots = list(range(2 * B))
cx = Context(0)
cx.set_params(params_from_tc(cfg2_context()))
cx.set_option(22, int(os.environ.get("LAZY", "1")))            # KLT_OPT_L0_LAZY_GRAD
if "FORM" in os.environ:
    cx.set_option(24, int(os.environ["FORM"]))                  # KLT_OPT_TRACK_LAZY_FORM
for i, (f0, f1) in enumerate(pairs):
    cx.upload(2 * i, f0)
    cx.upload(2 * i + 1, f1)
cx.build_pyramids_batch(slots)
for i in range(B):
    fl, placed = cx.select(2 * i, NFEAT, use_pyramid=True)
    assert placed == NFEAT
    cx.featbuf_upload(100 + i, fl)
h = hashlib.sha256()
for step in range(STEPS):
    cx.build_pyramids_batch(slots)
    lean = cx.level0_lean()
    cx.track_batch_async([(2 * i, 2 * i + 1, 100 + i, 200 + i) for i in range(B)], NFEAT)
    cx.sync()
    for i in range(B):
        h.update(cx.featbuf_download(200 + i, NFEAT).tobytes())
print("LAZY", os.environ.get("LAZY", "1"), "FORM", os.environ.get("FORM"), "lib", os.environ.get("KLT_GPU_LIB"), "last step lean:", lean, "records sha256", h.hexdigest())
cx.close()
