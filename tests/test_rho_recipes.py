"""CPU: the recipes of tests/support/problems.py RHO_RECIPES, on the oracle alone.  tests/test_gpu_rho_resume.py aims at the launches that follow a rho
update in the two-kernel on-chip form; whether an instance gets to them is decided by how often the oracle (and so the GPU) changes rho.  These
tests hold the recipes to what the GPU tests rely on, so that a change of a model or a seed cannot silently empty them."""
import numpy as np
import pytest

from tests.support import problems

RECIPES = sorted(problems.RHO_RECIPES)
UNSTABLE_CAP = 0.10          # share of a recipe's instances that may be left out of the comparison of iteration counts


@pytest.fixture(scope="module")
def counts(built):
    out = {}
    for rid in RECIPES:
        _, ls, _, st = problems.rho_recipe(rid)
        out[rid] = problems.oracle_rho_updates(ls, **st)
    return out


@pytest.mark.parametrize("rid", RECIPES)
def test_recipes_solve_and_reach_the_last_launch_pair(counts, rid):
    """per (recipe, MPCQP_RESUME_ROUNDS) pair of the GPU module: instances with >= rounds + 2 updates re-factorise in place"""
    _, ls, _, st = problems.rho_recipe(rid)
    assert (problems.oracle_solve(ls, nthreads=8, **st)["status"] == 1).all()
    _, _, _, _, rounds, half = problems.RHO_RECIPES[rid]
    assert rounds, rid
    for r in rounds:
        reach = counts[rid] >= r + 2
        assert reach.any(), (rid, r, np.bincount(counts[rid]))
        if half:
            assert 2 * reach.sum() >= ls.batch, (rid, r, np.bincount(counts[rid]))


@pytest.mark.parametrize("rid,rounds", [("q20", 1), ("q50", 1), ("cp100", 0), ("di60", 0), ("di60", 1)])
def test_recipes_mix_waiting_and_finished_instances(counts, rid, rounds):
    """some instances finish in an earlier launch: the later launches see waiting and finished instances side by side"""
    assert rounds in problems.RHO_RECIPES[rid][4]
    c = counts[rid]
    assert (c < rounds + 2).any() and (c >= rounds + 2).any(), (rid, rounds, np.bincount(c))


@pytest.mark.parametrize("rid", RECIPES)
def test_recipe_decisions_do_not_hang_on_rounding(built, rid):
    _, ls, _, st = problems.rho_recipe(rid)
    ok = problems.oracle_stable_mask(ls, **st)
    assert (~ok).sum() <= UNSTABLE_CAP * ls.batch, (rid, np.flatnonzero(~ok))


@pytest.mark.parametrize("rid", ["q20", "q50"])
def test_hand_over_edge_recipes(built, counts, rid):
    """what the edge cases of the GPU module rely on: iteration limits that fall on a rho update which parks the instance (the first at MPCQP_RESUME_ROUNDS = 0,
    the second at 1) or is served in place (the second at 0) for at least half of the batch, two halves of a batch that leave at different iterations
    (starting rho 0.1 / 10), a warm start that saves updates"""
    _, ls, _, st = problems.rho_recipe(rid)
    B = ls.batch
    for rounds, which, parks in problems.UPDATE_LIMIT_CASES:
        assert parks == (which + 1 <= rounds + 1)
        limits = problems.update_limits(ls, st, which)
        for mi in limits:
            s = dict(st, max_iter=mi)
            ref = problems.oracle_solve(ls, nthreads=8, **s)
            assert (ref["status"] == 7).all() and (ref["iters"] == mi).all()
            assert (~problems.oracle_stable_mask(ls, **s)).sum() <= UNSTABLE_CAP * B
            c, changed, interval = problems.oracle_rho_updates(ls, steps=True, **s)
            on_limit = changed[:, limits[0] // interval - 1] & (c == which + 1)         # its (which + 1)-th update, in the step of the limit
            assert 2 * on_limit.sum() >= B, (rounds, which, mi, c)
    rho0 = problems.split_rho(B)
    c = problems.oracle_rho_updates(ls, rho0=rho0, **st)
    assert 4 * (c[:B // 2] != c[B // 2:]).sum() >= B // 2, c
    assert 2 * (c >= 2).sum() >= B, c
    assert (~problems.oracle_stable_mask(ls, rho0=rho0, **st)).sum() <= UNSTABLE_CAP * B
    x0, y0, sw = problems.warm_point(ls, st)
    cw = problems.oracle_rho_updates(ls, x0=x0, y0=y0, **sw)
    assert cw.sum() < counts[rid].sum(), (cw, counts[rid])
    assert 2 * (cw >= 2).sum() >= B, cw
    assert (~problems.oracle_stable_mask(ls, x0=x0, y0=y0, **sw)).sum() <= UNSTABLE_CAP * B


@pytest.mark.parametrize("rid", ["q50", "cp100"])
def test_big_batch_samples_reach_the_last_launch_pair(built, rid):
    """the oracle sample of the batch that outnumbers the resident workgroups: at least half of it re-factorises in place at MPCQP_RESUME_ROUNDS = 0, some of it at 1"""
    ls, idx, st = problems.big_batch_sample(rid)
    c = problems.oracle_rho_updates(ls, **st)
    assert 2 * (c >= 2).sum() >= len(idx), np.bincount(c)
    if rid == "q50":
        assert 2 * (c >= 3).sum() >= len(idx) and (c < 3).any(), np.bincount(c)
    assert (~problems.oracle_stable_mask(ls, **st)).sum() <= UNSTABLE_CAP * len(idx)
