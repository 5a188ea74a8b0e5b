"""CPU side of tests/test_gpu_igemm_pointwise.py: the case list (tests/igemm_addr_cases.py) really contains the shapes its
docstring promises: which cases are eligible for the pointwise address form (takes_pointwise, which the GPU test checks against
the launcher's own count), how many k sub-steps a case has, whether a split leaves a slice empty."""
import igemm_addr_cases as ac

KS = {0: 1, 1: 2, 3: 1, 6: 2}                  # k sub-steps per step of the tile configs


def _substeps(c):
    cin_p, eps = ac.cin_stored(c), 64 if c["prec"] else 32
    return c["k"] * (-(-c["k"] * cin_p // 32) * 32) // eps


def _last_slice_is_empty(c):
    """the last slice begins at or behind the last step (slices take ceil(steps / splitk) steps each)"""
    steps = -(-_substeps(c) // KS[c["cfg"]])
    return (c["splitk"] - 1) * -(-steps // c["splitk"]) >= steps


def test_names_are_unique_and_groups_known():
    assert len({c["name"] for c in ac.CASES}) == len(ac.CASES)
    assert {c["group"] for c in ac.CASES} == set(ac.GROUPS)
    assert ac.LAUNCHES not in {c["name"] for c in ac.CASES}


def test_pointwise_group_takes_the_pointwise_form_and_covers_the_edges():
    pw = [c for c in ac.CASES if c["group"] == "pw"]
    assert all(ac.takes_pointwise(c) for c in pw)
    ms = {c["B"] * ((c["H"] - 1) // c["stride"] + 1) * ((c["W"] - 1) // c["stride"] + 1) for c in pw}
    assert {1, 63, 65, 129} <= ms
    assert {_substeps(c) for c in pw} >= {1, 2, 4}
    assert {c["cout"] for c in pw} == {64, 80} and {c["stride"] for c in pw} == {1, 2} and 3 in {c["B"] for c in pw}
    for cfg in ac.CFGS:
        mine = [c for c in pw if c["cfg"] == cfg]
        assert {c["splitk"] for c in mine} >= {0, 2, 3}
        assert any(_last_slice_is_empty(c) for c in mine if c["splitk"] > 1)
        # a dead part inside a split of two: one sub-step (at KS = 2 a live and a dead half step) in front of an empty slice, and
        # at KS = 2 also two sub-steps (one whole step) in front of one
        assert {_substeps(c) for c in mine if c["splitk"] == 2 and _last_slice_is_empty(c)} >= ({1, 2} if KS[cfg] == 2 else {1})
    assert {(c["res_mode"], c["relu"]) for c in pw} >= {(m, r) for m in (0, 1, 2) for r in (0, 1)}


def test_sixteen_bit_group_has_pointwise_and_general_cases():
    p16 = [c for c in ac.CASES if c["group"] == "pw16"]
    for prec in (1, 2):
        assert {ac.takes_pointwise(c) for c in p16 if c["prec"] == prec} == {True, False}
        assert {c["cfg"] for c in p16 if c["prec"] == prec and ac.takes_pointwise(c)} == set(ac.CFGS)


def test_general_group_keeps_the_general_code_on_every_small_map():
    g = [c for c in ac.CASES if c["group"] == "general"]
    assert not any(ac.takes_pointwise(c) for c in g)
    assert {_substeps(c) for c in g} >= {3, 5, 9}          # dead half steps behind live ones
    maps = {(h, w) for h in (1, 2, 5) for w in (1, 2, 5)} | {(9, 11)}
    for k in (3, 5, 7):
        for stride in (1, 2):
            assert {(c["H"], c["W"]) for c in g if c["k"] == k and c["stride"] == stride and c["cin"] == 32} >= maps
    k3 = [c for c in g if c["k"] == 3 and c["cin"] == 32]
    assert {c["cfg"] for c in k3} == set(ac.CFGS) and {c["splitk"] for c in k3} >= {0, 2, 4}
