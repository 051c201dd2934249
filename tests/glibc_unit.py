"""What tests/test_gpu_glibc_math.py and tests/test_cpu_glibc_math.py share: the
path of the unit programme of the libm replicas (tools/glibc_math_unit.hip,
built by csrc/Makefile with the library), the parser of its output lines

    name inputs=N subnormal_results=K ... device_vs_host=.. device_vs_libm=.. host_vs_libm=..

and the committed counts (tests/golden/glibc_math_unit_counts.json: per
function the exact size of its input set and the census of that set --
libm's subnormal, zero, infinite and NaN results, the inputs on each branch --
as `glibc_math_unit.bin host` printed them; the programme counts them from the
inputs and from libm's results, never from the code under test)."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = os.path.join(ROOT, "tools", "glibc_math_unit.bin")
GROUPS = {
    "float": ["expf", "logf", "log1pf"],
    "expf_t": ["expf_t", "expf_t_nonpos", "expf_t_le0", "expf_t_core"],
    "double": ["exp", "log"],
    "lse": ["lse_f32", "lse_f64"],
    "widen": ["widen_f16", "widen_bf16", "widen2_f16", "widen2_bf16"],
}
MISMATCH_KEYS = ("device_vs_host", "device_vs_libm", "host_vs_libm")

with open(os.path.join(ROOT, "tests", "golden", "glibc_math_unit_counts.json")) as _f:
    COUNTS = json.load(_f)


def parse(out):
    """{function: {key: value}} of the per-function lines, and the last line's
    (mismatches, inputs).  A mismatch count the mode does not compute ("-")
    parses as None."""
    lines = {}
    total = None
    for ln in out.splitlines():
        m = re.fullmatch(r"glibc_math_unit: (\d+) mismatches over (\d+) inputs", ln)
        if m:
            total = (int(m.group(1)), int(m.group(2)))
            continue
        t = ln.split()
        if len(t) < 2 or not t[1].startswith("inputs="):
            continue
        assert t[0] not in lines, ln
        lines[t[0]] = {k: (None if v == "-" else int(v)) for k, v in (x.split("=") for x in t[1:])}
    return lines, total


def check_counts(lines, names):
    """Every named function printed its line, over exactly the committed input
    set: the same size and the same census."""
    for name in names:
        assert name in lines, (name, sorted(lines))
        got = {k: v for k, v in lines[name].items() if k not in MISMATCH_KEYS}
        assert got == COUNTS[name], (name, got, COUNTS[name])
