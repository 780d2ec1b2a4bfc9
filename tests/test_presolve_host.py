"""The case table of tests/test_presolve_gpu.py against the oracle, on the CPU: every case really holds the sets of
instances its GPU test draws its evidence from (tests/model/presolve_cases.py), so that no GPU test passes vacuously --
and lambda_general / solo_limit restate what they claim to."""
import numpy as np
import pytest

from tests.model import presolve_cases as pc


@pytest.mark.parametrize("name", list(pc.CASES))
def test_case_meets_its_conditions(oracle, name):
    s = pc.solve_case(oracle, name)
    if pc.CASES[name]["form"] == "mixed":
        print(name, {H: (b.n, int(b.capped.sum()), int(b.spare.sum())) for H, (_, b) in s.items()})
        assert {H: b.n for H, (_, b) in s.items()} == pc.MIXED_BINS
    else:
        print(name, "n", s.n, "taken", int(s.taken.sum()), "capped", int(s.capped.sum()),
              "capped and not taken", int((s.capped & ~s.taken).sum()), "spare", int(s.spare.sum()))
    pc.check_conditions(name, s, cu_count=256)


def test_swapped_mixed_bins_hold_no_presolve_but_capped_instances(oracle):
    """The second mixed call of test_mixed_entry_under_auto: the same instances, 1000 at N = 40 and 4096 at N = 20; both
    bins still hold capped instances at max_iter = 2000."""
    hz, v, dy, dphi = pc.mixed_inputs(pc.MIXED_BINS_SWAPPED)
    assert len(hz) == sum(pc.MIXED_BINS.values())
    s = pc.solve_mixed(oracle, hz, v, dy, dphi, dict(max_iter=2000))
    assert {H: b.n for H, (_, b) in s.items()} == pc.MIXED_BINS_SWAPPED
    assert s[40][1].capped.any() and s[20][1].capped.any()


def test_lambda_general_is_the_compact_bound():
    """lambda_general on the compact model equals the scalar loop of test_capped_gpu.py (_lambda) written out here, and
    for I = 1 the hand-expanded sum."""
    H = 7
    v = np.array([0.1, 1.0, 2.5, 4.0])
    lam = pc.lambda_compact(v, H)
    for k, x in enumerate(v):
        a, c = pc.STEP * x, pc.STEP * x / pc.WHEELBASE
        A = np.array([[1.0, a], [0.0, 1.0]])
        B = np.array([[0.0, a], [c, -c]])
        Qd = np.diag(pc.WEIGHTS[:2]).astype(float)
        want, Tm = (pc.WEIGHTS[2] + pc.WEIGHTS[3]) * H, Qd.copy()
        for _ in range(H):
            want += np.trace(B.T @ Tm @ B)
            Tm = A.T @ Tm @ A + Qd
        assert abs(lam[k] - want) <= 1e-12 * want
    # I = 1, A = identity: Tm = (i + 1) diag(Q), trace(B' Tm B) = (i + 1) (q0 b0^2 + q1 b1^2)
    lam1 = pc.lambda_general([[1.0, 0.0, 0.0, 1.0]], [[0.5, 2.0]], [[3.0, 5.0]], [[0.25]], 4)
    assert lam1.shape == (1,) and lam1[0] == 4 * 0.25 + (1 + 2 + 3 + 4) * (3.0 * 0.25 + 5.0 * 4.0)


def test_solo_limit_restates_the_share():
    """7 of 16 SIMDs, 8 instances per wavefront: 3584 on a 256-CU part, and a presolve is tried up to five times that."""
    assert pc.solo_limit(256) == 3584 and pc.batch_bound(256) == 17920
    assert pc.solo_limit(64) == 896
    assert pc.threshold(2000) == (2000 / 7.0) ** 2
