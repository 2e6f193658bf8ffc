"""The QK-norm kernel's host-visible code under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU:
csrc/tests/qk_norm_check.cpp (its own ``main``; nothing is preloaded) runs the launch plan of csrc/qk_norm_plan.h
on every shape of the kernel tests, every refusal code, and the launcher of csrc/qk_norm_rope.hip, which returns
the plan's code before any HIP call.

The case file is whitespace-separated integers, one ``T Hq Hkv D grid`` record per case: one wave per (token,
head slot), four waves per workgroup."""
import os
import shutil
import subprocess

import pytest

from theroundtaible_amd.ops import oracle64 as o64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def grid_cases():
    rows = []
    for hq, hkv, D in o64.QKNORM_SHAPES:
        for T in o64.QKNORM_T + (16, 4096):
            rows.append((T, hq, hkv, D, -(-T * (hq + 2 * hkv) // 4)))
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_qk_norm_plan_and_launcher_under_asan_ubsan(tmp_path):
    rows = grid_cases()
    assert (3, 32, 8, 128, 36) in rows and (1, 1, 1, 64, 1) in rows       # 144 waves; 3 waves in one workgroup
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(" ".join(str(v) for v in r) for r in rows))
    exe = str(tmp_path / "qk_norm_check")
    srcs = [os.path.join(CSRC, "tests", "qk_norm_check.cpp"), os.path.join(CSRC, "qk_norm_rope.hip")]
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", CSRC, *srcs, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    nm = shutil.which("nm")
    if nm:
        syms = subprocess.run([nm, exe], capture_output=True, text=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms   # the sanitizers really are linked in
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"{len(rows)} grids, 0 failure(s)" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
