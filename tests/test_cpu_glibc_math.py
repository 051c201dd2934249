"""The glibc replicas the kernels compute with (csrc/glibc_math.h: expf, logf,
log1pf and the normalisers' expf_t_nonpos / expf_t_le0 / expf_t_core;
csrc/glibc_math_f64.h: exp, log) against the host libm, through their
stand-alone checkers in tools/: compiled for the host with the documented
line (-ffp-contract=off, as the device code) and run CI-sized.  The GPU tests
compare kernels with the oracle, whose exp and log are the host libm's; this
is the other half, that the headers themselves agree with that libm, over
every 97th float pattern and two million samples per double domain."""
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
