"""The glibc replicas the kernels compute with (csrc/glibc_math.h: expf, logf,
log1pf and the normalisers' expf_t_nonpos / expf_t_le0 / expf_t_core;
csrc/glibc_math_f64.h: exp, log) against the host libm, through their
stand-alone checkers in tools/: compiled for the host with the documented
line (-ffp-contract=off, as the device code) and run CI-sized.  The GPU tests
compare kernels with the oracle, whose exp and log are the host libm's; this
is the other half, that the headers themselves agree with that libm, over
every 97th float pattern and two million samples per double domain.

test_unit_programme_host_mode runs the host mode of the unit programme of the
device check (tools/glibc_math_unit.hip, tests/test_gpu_glibc_math.py): the
same input sets as on the GPU, the host pass of the header functions against
libm, and the sizes and census of the input sets against the committed
counts.  That is how the sets -- the subnormal-result band of expf, the bands
around every branch constant, lse's pairs -- are verified without a GPU."""
import os
import re
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = str(min(16, os.cpu_count() or 1))


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _build(src, out):
    subprocess.run([_hipcc(), "-O2", "-ffp-contract=off", "-std=c++17", os.path.join(ROOT, "tools", src), "-o", out,
                    "-lpthread"], check=True, cwd=ROOT, timeout=600)


def _run(*cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    return r.stdout


def test_float_replicas_match_libm(tmp_path):
    chk = str(tmp_path / "chk")
    _build("check_glibc_math.cpp", chk)
    out = _run(chk, "sample", THREADS)
    lines = out.strip().splitlines()
    assert len(lines) == 1, out      # (a mismatch prints the input before the summary)
    m = re.fullmatch(r"stride=97 mismatches: expf=(\d+) logf=(\d+) log1pf=(\d+) expf_t_nonpos=(\d+)", lines[0])
    assert m and [int(g) for g in m.groups()] == [0, 0, 0, 0], out


def test_double_replicas_match_libm(tmp_path):
    chk = str(tmp_path / "chk64")
    _build("check_glibc_math_f64.cpp", chk)
    out = _run(chk, "2000000", THREADS)
    lines = out.strip().splitlines()
    assert len(lines) == 10, out     # one line per domain
    for ln in lines:
        m = re.fullmatch(r"(exp|log) .*\S\s+(\d+) samples, (\d+) mismatches", ln)
        assert m and int(m.group(2)) == 2000000 and int(m.group(3)) == 0, out


def test_unit_programme_host_mode():
    import pytest

    from glibc_unit import COUNTS, GROUPS, UNIT, check_counts, parse
    hipcc = _hipcc()
    if not (shutil.which(hipcc) or os.path.exists(hipcc)):
        pytest.skip("hipcc is absent: tools/glibc_math_unit.bin cannot be built")
    # the way build() makes it: csrc/Makefile's rule, with the library's flags
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ctc-beam-search-op_amd", "csrc"), "HIPCC=" + hipcc,
                    os.path.join("..", "..", "tools", "glibc_math_unit.bin")], check=True, timeout=600)
    lines, total = parse(_run(UNIT, "host"))
    assert sorted(lines) == sorted(COUNTS), sorted(lines)
    for group in GROUPS.values():
        check_counts(lines, group)
    for name, ln in lines.items():
        assert ln["host_vs_libm"] == 0 and ln["device_vs_host"] is None and ln["device_vs_libm"] is None, (name, ln)
    assert total == (0, sum(c["inputs"] for c in COUNTS.values())), total
    # the committed sizes against the sets as the issue of the check states them
    band = 0xc2cff1b4 - 0xc2aeac50 + 1          # expf's subnormal results: [kExpfUnder, log(2^-126))
    assert band == 2180453
    floats = -(-2**32 // 97) + (band + 128) + 2 * 2**23 + (13 + 3 + 4) * 8193
    assert COUNTS["expf"]["inputs"] == COUNTS["logf"]["inputs"] == COUNTS["expf_t"]["inputs"] == floats
    assert COUNTS["log1pf"]["inputs"] == floats + 0x3f800000 // 13 + 1
    for name in GROUPS["expf_t"] + ["expf"]:     # the whole band, and the sampled patterns that fall in it
        assert COUNTS[name]["subnormal_results"] >= band, name
    assert COUNTS["exp"]["inputs"] == 5 * 2000000 + 6 * 8193
    assert COUNTS["log"]["inputs"] == 5 * 2000000 + 4 * 8193 + 4097
    pairs = (0xc2d1f1b4 - 0x80000000) // 41 + 1   # d: every 41st pattern of [kExpfUnder - 1, -0]
    assert COUNTS["lse_f32"]["inputs"] == COUNTS["lse_f64"]["inputs"] == 2 * (pairs + 25)
    assert COUNTS["widen_f16"]["inputs"] == COUNTS["widen_bf16"]["inputs"] == 65536
    assert COUNTS["widen2_f16"]["inputs"] == COUNTS["widen2_bf16"]["inputs"] == 2 * 65536
