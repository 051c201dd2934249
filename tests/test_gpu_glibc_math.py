"""The libm replicas as the gfx950 compile of the kernel source runs them
(csrc/glibc_math.h: expf, logf, log1pf, expf_t with its table in LDS and the
branch-free expf_t_nonpos / expf_t_le0 / expf_t_core; csrc/glibc_math_f64.h:
exp, log with their tables in constant memory; lse<float> and lse<double>, the
composite of every beam update; the fp16 / bf16 widenings), function by
function, one input per thread, against the host pass of the same functions
and against the host libm, bit for bit.

The unit programme (tools/glibc_math_unit.hip) includes ctcx_decode.hip itself
and csrc/Makefile builds it with the library's own $(FLAGS), so what runs here
is what the kernels run: a dropped -ffp-contract=off, flushed f32 denormals, a
compiler that rounds log1pf's divisions or v_cvt_f32_f64 differently, or a
rewrite of one expression moves a bit here whether or not a parity case
happens to reach the input.  (Built once without -ffp-contract=off the
programme reported 17,969 log1pf, 504 exp, 3,268 lse<float> and 6,054
lse<double> device-against-host mismatches; built with flushed denormals,
2,211,125 in each expf form, 8,475,087 in logf, 15,206 and 11,830 in lse.)

The programme runs once per session (about 2 s).  Each test asserts for its
functions that device-against-host, device-against-libm and host-against-libm
mismatches are all 0, and that the input set is the committed one: its exact
size and its census (tests/golden/glibc_math_unit_counts.json, verified
without a GPU by tests/test_cpu_glibc_math.py), so a case cannot pass without
the subnormal results and branch inputs it exists for."""
import functools
import os
import subprocess

import pytest

from glibc_unit import COUNTS, GROUPS, MISMATCH_KEYS, UNIT, check_counts, parse

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _run():
    assert os.path.exists(UNIT), "tools/glibc_math_unit.bin is missing: build() makes it with the library"
    r = subprocess.run(["timeout", "-k", "10", "120", UNIT], capture_output=True, text=True)
    print(r.stdout)
    lines, total = parse(r.stdout)
    return r, lines, total


def _check(group):
    r, lines, _ = _run()
    assert r.returncode in (0, 1), r.stdout + r.stderr   # (1: mismatches, reported below by function)
    check_counts(lines, GROUPS[group])
    for name in GROUPS[group]:
        assert [lines[name][k] for k in MISMATCH_KEYS] == [0, 0, 0], (name, lines[name], r.stdout)


def test_programme_ran_clean():
    r, lines, total = _run()
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(lines) == sorted(COUNTS), sorted(lines)
    assert total == (0, sum(c["inputs"] for c in COUNTS.values())), r.stdout


def test_float_functions():
    _check("float")


def test_expf_table_forms():
    _check("expf_t")


def test_double_functions():
    _check("double")


def test_lse():
    _check("lse")


def test_widenings():
    _check("widen")
