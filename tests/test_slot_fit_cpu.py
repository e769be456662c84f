"""What the segment sort's scatter may take of a CU, so that its waves fit beside a running align launch.

A streamed launch of the lean exact DIRECT7 body leaves thirds of a CU to the next batch's target build: beside two lean workgroups -- 168 VGPRs
and 45,568 B of LDS each, quoted from DESIGN.md section 4.1, not recompiled here -- a SIMD has 512 - 2 * 168 = 176 VGPRs free and the CU
163,840 - 2 * 45,568 = 72,704 B of LDS.  A two-wave launch leaves halves of a CU: 256 VGPRs per SIMD.  `k_rs_scatter` used to need 137 VGPRs:
ONE wave per SIMD in either slot, against two VALU-saturating align waves.  Its budgets:

  digit widths 8 and 10, FIRST both ways:  <= 56 VGPRs (3 x 56 <= 176), <= 24,232 B of LDS per block (3 x that <= 72,704), no scratch
                                           -> three waves per SIMD in a lean slot, four in a half-CU slot
  width 11 (the run table alone is 32 KB):  <= 88 VGPRs, <= 36,352 B of LDS, no scratch -> two waves per SIMD

The test compiles tools/segsort_res.hip (the segment sort's kernels, device code only) with the library's own flags and reads the compiler's
kernel-resource-usage remarks through tools/slot_fit.py.  No GPU; skipped where hipcc is absent.
"""
import importlib.util
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def _slot_fit():
    spec = importlib.util.spec_from_file_location("slot_fit", os.path.join(ROOT, "tools", "slot_fit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(entry.HIPCC):
        pytest.skip("hipcc not found")
    sf = _slot_fit()
    flags = [f for f in entry.HIP_FLAGS if f not in ("-fPIC", "-shared")]
    cmd = [entry.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", os.path.join(ROOT, "tools", "segsort_res.hip"), "-o", os.devnull]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = sf.parse(p.stderr)
    names = list(rows)
    return sf, dict(zip(sf.demangle(names), (rows[n] for n in names)))


@pytest.mark.parametrize("first", ["false", "true"])
@pytest.mark.parametrize("bits", [8, 10])
def test_scatter_fits_three_times_into_a_lean_slot(kernels, bits, first):
    sf, k = kernels
    r = k[f"k_rs_scatter<{bits}, {first}>"]
    print(bits, first, r)
    assert r["VGPRs"] + r["AGPRs"] <= 56
    assert r["LDS Size [bytes/block]"] <= 24232
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0
    assert sf.waves_in_slot(r, "lean") >= 3
    assert sf.waves_in_slot(r, "half-CU") >= 4


@pytest.mark.parametrize("first", ["false", "true"])
def test_widest_scatter_fits_twice(kernels, first):
    sf, k = kernels
    r = k[f"k_rs_scatter<11, {first}>"]
    print(first, r)
    assert r["VGPRs"] + r["AGPRs"] <= 88
    assert r["LDS Size [bytes/block]"] <= 36352
    assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0
    assert sf.waves_in_slot(r, "lean") >= 2
    assert sf.waves_in_slot(r, "half-CU") >= 2


def test_slot_arithmetic():
    """the model itself, on the figures of the kernels as they stood before: one scatter wave in either slot, k_rank's sixteen-wave block in neither lean slot"""
    sf = _slot_fit()
    old_scatter = {"VGPRs": 137, "AGPRs": 0, "LDS Size [bytes/block]": 16384}
    assert sf.waves_in_slot(old_scatter, "lean") == 1 and sf.waves_in_slot(old_scatter, "half-CU") == 1
    assert sf.waves_in_slot({"VGPRs": 61, "AGPRs": 0, "LDS Size [bytes/block]": 68}, "lean", threads=1024) == 0
    assert sf.waves_in_slot({"VGPRs": 61, "AGPRs": 0, "LDS Size [bytes/block]": 68}, "half-CU", threads=1024) == 4
    assert sf.waves_in_slot({"VGPRs": 42, "AGPRs": 0, "LDS Size [bytes/block]": 18432}, "lean") == 3          # k_leafsum
    assert sf.waves_in_slot({"VGPRs": 36, "AGPRs": 0, "LDS Size [bytes/block]": 16384}, "lean") == 4          # k_rs_hist<10, true>
    assert sf.waves_in_slot({"VGPRs": 64, "AGPRs": 0, "LDS Size [bytes/block]": 96}, "lean") == 2             # k_minmax at four loads in flight
