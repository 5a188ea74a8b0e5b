"""-m gpu: the pointwise address form of conv_igemm_f32's k loop (csrc/conv_igemm.hip, conv_igemm_f32<.., apse_pointwise>) against the
general per-step address code of the same build, through the stateless apse_conv2d.

The form moves address arithmetic out of the loop and into the buffer instructions' scalar offset; it issues the same loads of
the same bytes, so every output must be BYTE-IDENTICAL to the general code's -- there is no tolerance.  The switch
APSE_IGEMM_ADDR is read once per process, so tests/igemm_addr_cases.py runs every case in a fresh child process per setting
(two children in all) and this module compares the bytes they wrote.  Each child also reports, per case, how many launches took
the pointwise kernel (apse_conv_pointwise_launches): exactly one for every eligible case under APSE_IGEMM_ADDR=1, none anywhere
under APSE_IGEMM_ADDR=0 -- so the comparison cannot pass by running the same kernel twice.

Cases (tests/igemm_addr_cases.py), the smallest shapes at which the address code can go wrong:
* 1x1 at stride 1 and 2; Cin 32 / 64 / 96 stored as 128 (1, 2, 4 sub-steps: the dead half of a KS = 2 step, one step, two);
  Cout 64 and 80 (columns past the tile); M = 1, 63, 65, 129 (rows past M in the first and in the last tile); split K 2 and 3 with
  an empty slice, and Cin 32 / 64 split in two (a dead half step and an empty slice inside one split); B = 3; residual modes
  0 / 1 / 2 with ReLU on and off; tile configs 0, 1, 3, 6; bf16 / f16 operands and storage.
  A pointwise filter row is Cin, a power of two, so 3 and 5 sub-steps (a dead half step behind live ones) exist only for the
  padded filters below: 3x3 over Cin 8 and 5x5 over Cin 4.
* 3x3 / pad 1, 5x5 / pad 2 and 7x7 / pad 3 at stride 1 and 2 on maps of 1, 2 and 5 pixels a side and 9 x 11: every pattern of
  taps inside and outside the map.  They keep the general code under both settings and pin that the switch leaves them alone.
Every operand lies between NaN guard bands and y and the workspace are NaN-filled; the worker asserts the bands and that no NaN
reached y.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import igemm_addr_cases as ac

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(tmp, setting):
    path = os.path.join(tmp, "addr%s.npz" % setting)
    env = dict(os.environ, APSE_IGEMM_ADDR=setting)
    child = subprocess.run([sys.executable, os.path.join(HERE, "igemm_addr_cases.py"), path], capture_output=True, text=True, env=env)
    assert child.returncode == 0, "APSE_IGEMM_ADDR=%s: %s" % (setting, (child.stdout[-2000:] + child.stderr[-4000:]))
    with np.load(path) as z:
        return {k: z[k] for k in z.files if k != ac.LAUNCHES}, [int(v) for v in z[ac.LAUNCHES]]


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("igemm_addr"))
    return _child(tmp, "1"), _child(tmp, "0")


@pytest.mark.parametrize("group", ac.GROUPS)
def test_address_forms_keep_the_general_codes_bytes(outputs, group):
    (new, _), (general, _) = outputs
    names = [c["name"] for c in ac.CASES if c["group"] == group]
    assert names
    bad = []
    for n in names:
        a, b = new[n], general[n]
        assert a.shape == b.shape and a.size > 0, n
        if not np.array_equal(a, b):
            bad.append((n, int((a != b).sum()), a.size))
    print(group, len(names), "cases,", len(bad), "differ")
    assert not bad, "bytes differ from the general address code (case, differing bytes, bytes): %s" % bad[:12]


def test_every_case_ran_in_both_processes(outputs):
    (new, _), (general, _) = outputs
    assert sorted(new) == sorted(general) == sorted(c["name"] for c in ac.CASES)


def test_the_pointwise_kernel_ran_where_it_should_and_nowhere_else(outputs):
    (_, new_launches), (_, general_launches) = outputs
    want = [1 if ac.takes_pointwise(c) else 0 for c in ac.CASES]
    assert sum(want) > 0
    wrong = [(c["name"], got, w) for c, got, w in zip(ac.CASES, new_launches, want) if got != w]
    assert not wrong and len(new_launches) == len(want), "pointwise launches under APSE_IGEMM_ADDR=1 (case, got, expected): %s" % wrong[:12]
    assert general_launches == [0] * len(ac.CASES), "APSE_IGEMM_ADDR=0 launched the pointwise kernel"
