"""The Frenet helpers take cos and sin of one angle from a single sincos (emp_frenet_core.h, sincos_pair): on the device it must
return what the separate sin and cos calls return, bit for bit, or every projection and trajectory point could move."""
import os
import shutil
import subprocess

import pytest


@pytest.mark.gpu
def test_device_sincos_equals_sin_and_cos_bit_for_bit(tmp_path):
    """tools/sincos_bits_test.hip compares sincos(x) with sin(x) and cos(x) on 1.07e9 operands - an even sweep of [-4 pi, 4 pi], a
    hashed sweep over every exponent, denormals, +-0, +-inf, NaN, multiples of pi / 2 and their neighbours: no result may differ."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "sincos_bits_test")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                            os.path.join(root, "tools", "sincos_bits_test.hip"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "sincos differing from sin / cos: 0" in run.stdout, run.stdout + run.stderr
