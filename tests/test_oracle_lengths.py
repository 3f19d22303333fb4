"""The CPU oracle at TimeLimits and plan lengths other than 200, pinned to the reference.

tests/golden/bb_lengths.npz (make_golden.py "lengths") holds BlackBoxWrapper runs of the reference's
own code with TimeLimit(env, M), spec.max_episode_steps = M and a stub generator of T samples.  The
per-env port and the vectorised oracle reproduce them bit for bit with max_episode_steps=M.
"""
import os

import numpy as np
import pytest

from oracle import batched, port

# prefix: env, controller (port, batched), M, T, replan period
CASES = {
    "len_long": ("LongSimpleReacher", lambda: port.PD(0.6, 0.075), ("pd", 0.6, 0.075), 252, 252, 0),
    "len_hole": ("HoleReacher", lambda: port.PD(1.0, 0.1), ("pd", 1.0, 0.1), 252, 252, 0),
    "len_replan": ("SimpleReacher", lambda: port.PD(1.0, 0.1), ("pd", 1.0, 0.1), 120, 120, 25),
}


@pytest.fixture(scope="module")
def lengths(golden_dir):
    return np.load(os.path.join(golden_dir, "bb_lengths.npz"))


def _table_traj(pos_t, vel_t, T):
    def fn(params, init_time, cpos, cvel):
        t0 = int(round(init_time / 0.01))
        return pos_t[t0:t0 + T].copy(), vel_t[t0:t0 + T].copy()
    return fn


def test_fixture_shapes(lengths):
    """The fixture holds what the cases are about: full 252-sample episodes, both outcomes on
    HoleReacher, and a 20-sample last segment that truncates at the TimeLimit of 120."""
    g = lengths
    assert g["len_long_ret"].shape == (8, 2) and g["len_hole_ret"].shape == (8, 2)
    assert g["len_replan_ret"].shape == (8, 6)
    assert np.all(g["len_long_tlen"] == 252) and np.all(g["len_long_trunc"]) and not np.any(g["len_long_term"])
    assert g["len_long_step_rew"].shape == (8, 2, 252)
    assert np.all((g["len_hole_tlen"] == 252) == g["len_hole_trunc"])
    assert np.array_equal(g["len_replan_tlen"], np.tile([25, 25, 25, 25, 20, 25], (8, 1)))
    assert np.array_equal(g["len_replan_trunc"], np.tile([0, 0, 0, 0, 1, 0], (8, 1)).astype(bool))


def test_reference_return_is_np_sum_of_252(lengths):
    """black_box_wrapper.py:252 aggregates with np.sum: the recorded returns are np.sum of the
    recorded step rewards, so the fixture itself witnesses numpy's order for 252 terms (split at
    120, the 132-term second half split again at 64).  A sum that keeps the second half in one
    block differs on these rows."""
    g = lengths
    rew, ret, tlen = g["len_long_step_rew"], g["len_long_ret"], g["len_long_tlen"]
    one_level = 0
    for i in range(rew.shape[0]):
        for b in range(rew.shape[1]):
            L = tlen[i, b]
            assert L == 252
            assert ret[i, b] == np.sum(rew[i, b, :L])
            # the sum with an unsplit second half (what a one-level "first + rest" gives)
            r = rew[i, b, :L]
            one_level += (np.sum(r[:120]) + _block(r[120:])) != ret[i, b]
    assert one_level > 0, "no row of the fixture tells the two orders apart"


def _block(x):
    """One unsplit numpy pairwise block over x (any length): 8 accumulators, then the tail."""
    n = len(x)
    r = [x[j] for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + x[i + j]
        i += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for j in range(i, n):
        s = s + x[j]
    return s


@pytest.mark.parametrize("case", list(CASES))
def test_port_vs_golden(lengths, case):
    g = {k[len(case) + 1:]: lengths[k] for k in lengths.files if k.startswith(case + "_")}
    name, ctrl, _, M, T, replan = CASES[case]
    E, n_bb = g["ret"].shape
    for i in range(E):
        env = port.Reacher(name, max_episode_steps=M)
        bb = port.BlackBoxPort(env, _table_traj(g["pos"][i], g["vel"][i], T), ctrl(), replan_period=replan)
        np.testing.assert_array_equal(bb.reset(seed=100 + i), g["obs0"][i])
        for b in range(n_bb):
            assert bb.traj_steps * 0.01 == pytest.approx(g["init_time"][i, b]) or replan == 0
            np.testing.assert_array_equal(env.q, g["init_pos"][i, b])
            np.testing.assert_array_equal(env.qd, g["init_vel"][i, b])
            obs, ret, te, tr, info = bb.step()
            L = info["trajectory_length"]
            assert L == g["tlen"][i, b]
            assert bool(te) == g["term"][i, b] and bool(tr) == g["trunc"][i, b]
            assert ret == g["ret"][i, b], (i, b, ret, g["ret"][i, b])
            np.testing.assert_array_equal(obs, g["obs"][i, b])
            np.testing.assert_array_equal(info["step_actions"], g["actions"][i, b, :L])
            np.testing.assert_array_equal(info["step_observations"], g["step_obs"][i, b, :L])
            np.testing.assert_array_equal(info["step_rewards"], g["step_rew"][i, b, :L])
            if name == "HoleReacher":
                np.testing.assert_array_equal(np.array(info["is_collided"], float), g["info_a"][i, b, :L])
                np.testing.assert_array_equal(np.array(info["is_success"], float), g["info_b"][i, b, :L])
                np.testing.assert_array_equal(np.array(info["end_effector"]), g["info_ee"][i, b, :L])
            else:
                np.testing.assert_array_equal(np.array(info["reward_dist"], float), g["info_a"][i, b, :L])
                np.testing.assert_array_equal(np.array(info["reward_ctrl"], float), g["info_b"][i, b, :L])
            if replan:   # TimeAwareObservation: the last column is t / max_episode_steps
                t = np.arange(bb.t_aware - L + 1, bb.t_aware + 1)
                np.testing.assert_array_equal(info["step_observations"][:, -1], (t / M).astype(np.float32))
            if te or tr:
                np.testing.assert_array_equal(bb.reset(), g["reset_obs"][i, b])


@pytest.mark.parametrize("case", list(CASES))
def test_batched_vs_golden(lengths, case):
    g = {k[len(case) + 1:]: lengths[k] for k in lengths.files if k.startswith(case + "_")}
    name, _, ctrl, M, T, replan = CASES[case]
    E, n_bb = g["ret"].shape
    P, V = g["pos"], g["vel"]

    def traj(params, s0, q, qd):
        rows = s0[:, None] + np.arange(T)[None, :]
        return P[np.arange(E)[:, None], rows], V[np.arange(E)[:, None], rows]

    bb = batched.BatchedBB(name, E, ctrl, traj_fn=traj, replan_period=replan, info_level=2, max_episode_steps=M)
    np.testing.assert_array_equal(bb._reset_idx(list(range(E)), [100 + i for i in range(E)]), g["obs0"])
    for b in range(n_bb):
        obs, ret, te, tr, info = bb.step(None)
        np.testing.assert_array_equal(info["trajectory_length"], g["tlen"][:, b])
        np.testing.assert_array_equal(te, g["term"][:, b])
        np.testing.assert_array_equal(tr, g["trunc"][:, b])
        np.testing.assert_array_equal(ret, g["ret"][:, b])
        np.testing.assert_array_equal(info["final_obs"], g["obs"][:, b])
        done = te | tr
        np.testing.assert_array_equal(obs[done], g["reset_obs"][:, b][done])
        for i in range(E):
            L = g["tlen"][i, b]
            np.testing.assert_array_equal(info["step_actions"][i, :L], g["actions"][i, b, :L])
            np.testing.assert_array_equal(info["step_observations"][i, :L], g["step_obs"][i, b, :L])
            np.testing.assert_array_equal(info["step_rewards"][i, :L], g["step_rew"][i, b, :L])


def test_table_rows_follow_the_time_limit():
    """With replanning the tables span the TimeLimit plus one plan: (M if do_replan else 0) + T + 2."""
    from oracle import mp
    spec = mp.MPSpec("prodmp", 2, 5, "exp", 1.5, alpha=10.0, duration=1.2)
    for M, replan, rows in ((120, 25, 242), (120, 0, 122), (200, 25, 322)):
        bb = batched.BatchedBB("SimpleReacher", 2, ("pd", 1.0, 0.1), mp_spec=spec, replan_period=replan,
                               max_episode_steps=M)
        assert next(iter(bb.tables.values())).shape[0] == rows, (M, replan)
