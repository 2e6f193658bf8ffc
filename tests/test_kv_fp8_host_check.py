"""The FP8 K/V cache's host-visible code under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU:
csrc/tests/kv_fp8_check.cpp (its own ``main``; nothing is preloaded) runs the scalar rule of csrc/kv_fp8_core.h —
the copy every cache writer runs — against ops/reference.py, and checks the fp8 block layouts, the decode
attention plan with an fp8 cache and the fp8 launchers' argument validation, which rejects before any HIP call.

The case file is whitespace-separated integers: the number of inverse scales; per inverse scale its fp32 bits,
then the expected code of every finite bf16 bit pattern in ascending order of the pattern; then the fp32 bits of
the value of each of the 256 codes (-1: NaN)."""
import os
import shutil
import subprocess

import pytest
import torch

from theroundtaible_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SCALES = (1.0, 4.0, 0.37)          # inverse scales 1, 0.25, 1 / 0.37


def finite_bf16() -> torch.Tensor:
    bits = torch.arange(65536, dtype=torch.int64)
    finite = ((bits >> 7) & 0xFF) != 0xFF
    signed = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)      # the same 16 bits
    y = signed[finite].view(torch.bfloat16).float()
    assert y.numel() == 65280 and bool(torch.isfinite(y).all())
    return y


def rule_cases():
    y = finite_bf16()
    nums = [len(SCALES)]
    for s in SCALES:
        inv = ref.kv_fp8_inv(s)
        nums.append(int(inv.view(torch.int32)))
        codes = ref.kv_fp8_code(y, inv)
        assert codes.dtype == torch.uint8 and int(codes.max()) <= 0xFE
        nums += codes.tolist()
    vals = ref.kv_fp8_value(torch.arange(256, dtype=torch.int64).to(torch.uint8))
    for c, v in enumerate(vals):
        nums.append(-1 if torch.isnan(v) else int(v.view(torch.int32)) & 0xFFFFFFFF)
        assert bool(torch.isnan(v)) == (c & 0x7F == 0x7F)
    return nums, y.numel() * len(SCALES)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_kv_fp8_rule_layout_plan_and_launchers_under_asan_ubsan(tmp_path):
    nums, n_codes = rule_cases()
    path = tmp_path / "cases.txt"
    path.write_text(" ".join(str(int(n)) for n in nums))
    exe = str(tmp_path / "kv_fp8_check")
    srcs = [os.path.join(CSRC, "tests", "kv_fp8_check.cpp")] + [
        os.path.join(CSRC, f) for f in ("attention_decode.hip", "attention_prefill.hip", "attention_prefill32.hip",
                                        "rope_cache.hip", "gemm_skinny.hip")]
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", CSRC, *srcs, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert b.returncode == 0, b.stderr[-3000:]
    nm = shutil.which("nm")
    if nm:
        syms = subprocess.run([nm, exe], capture_output=True, text=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms   # the sanitizers really are linked in
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"{n_codes} codes, 256 values, 0 failure(s)" in r.stdout
    assert n_codes == 3 * 65280
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
