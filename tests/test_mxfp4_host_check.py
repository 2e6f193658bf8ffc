"""The MXFP4 path's host-visible code under AddressSanitizer + UndefinedBehaviorSanitizer, without a GPU:
csrc/tests/fp4_check.cpp (its own ``main``; nothing is preloaded) runs the scalar rule of csrc/fp4_core.h —
the copy the quantise / dequantise kernels run — against ops/reference.py, and checks the lane-record map for
the 128-deep records, the launch plan, ``weight_shape_ok`` and the launchers' argument validation, which
rejects before any HIP call.

The case file is whitespace-separated integers: the number of scale bytes; per scale byte ``e``, the expected
code of every finite bf16 bit pattern in ascending order of the pattern, then the bf16 bits of the value of each
of the 16 codes; then the number of amax cases and per case the fp32 bits of ``amax`` + the expected scale byte."""
import os
import shutil
import subprocess

import pytest
import torch

from theroundtaible_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
SCALE_BYTES = (2, 100, 127, 140, 252)


def code_cases():
    bits = torch.arange(65536, dtype=torch.int64)
    finite = ((bits >> 7) & 0xFF) != 0xFF
    signed = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16)      # the same 16 bits
    wf = signed[finite].view(torch.bfloat16).float()
    assert wf.numel() == 65536 - 256 and bool(torch.isfinite(wf).all())
    nums = [len(SCALE_BYTES)]
    for e in SCALE_BYTES:
        nums.append(e)
        codes = ref.mxfp4_code(wf, torch.tensor(e, dtype=torch.int32))
        assert set(codes.tolist()) == set(range(16))
        nums += codes.tolist()
        # the value of each code: one byte holds codes (c, c), dequantised under e
        packed = torch.arange(16, dtype=torch.uint8).repeat_interleave(16)[None, :] * 17
        vals = ref.dequantize_mxfp4(packed.contiguous(), torch.full((1, 16), e, dtype=torch.uint8))[0, ::32]
        assert torch.isfinite(vals.float()).all()
        nums += (vals.view(torch.int16).int() & 0xFFFF).tolist()
    return nums, wf.numel() * len(SCALE_BYTES)


def scale_cases():
    g = torch.Generator().manual_seed(7)
    bits = [0, 1, 0x7FFFFF]                                  # zero and the fp32 subnormals: exponent field 0
    for E in range(1, 255):
        bits += [E << 23, (E << 23) | 1, (E << 23) | 0x7FFFFF, (E << 23) | int(torch.randint(1 << 23, (1,), generator=g))]
    amax = torch.tensor(bits, dtype=torch.int32).view(torch.float32)
    e = ref.mxfp4_scale_byte(amax)
    assert int(e.min()) == 2 and int(e.max()) == 252 and e[0].item() == 2
    nums = [len(bits)]
    for b, want in zip(bits, e.tolist()):
        nums += [b, want]
    return nums, len(bits)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fp4_rule_layout_plan_and_launchers_under_asan_ubsan(tmp_path):
    codes, n_codes = code_cases()
    scales, n_scales = scale_cases()
    path = tmp_path / "cases.txt"
    path.write_text(" ".join(str(int(n)) for n in codes + scales))
    exe = str(tmp_path / "fp4_check")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
           "-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I", CSRC, os.path.join(CSRC, "tests", "fp4_check.cpp"), os.path.join(CSRC, "gemm_skinny.hip"),
           os.path.join(CSRC, "gemm_skinny_fp4.hip"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert b.returncode == 0, b.stderr[-3000:]
    nm = shutil.which("nm")
    if nm:
        syms = subprocess.run([nm, exe], capture_output=True, text=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms   # the sanitizers really are linked in
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"{n_codes} codes, {n_scales} scale bytes, 20 layouts, 0 failure(s)" in r.stdout
    assert n_codes == 5 * 65280 and n_scales > 1000
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
