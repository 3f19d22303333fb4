"""GPU parity: libfgx.so (HIP, gfx950) vs the CPU oracle and the reference-generated goldens.

Tolerances (north_star): terminated / truncated flags, trajectory lengths and every integer of
the state are compared bit-exactly; f32 observations and f64 returns within 1e-5 relative.
Bit-exact equality is additionally required where the computation is exactly specified on both
sides (env state after reset, MP trajectories given the tables, actions).
"""
import os

import numpy as np
import pytest
import torch

import fancy_gym_crowd_amd as fgx
from oracle import batched, mp, port

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-5


def np_(t):
    return t.detach().cpu().numpy()


def kernel_is(got, want):
    """episode kernel name check (env.episode_kernel(), fgx_select.h)"""
    return got == want


def close(a, b, rtol=RTOL, atol=1e-6):
    np.testing.assert_allclose(np.asarray(a, np.float64), np.asarray(b, np.float64), rtol=rtol, atol=atol)


NAME = {"SimpleReacher-v0": "SimpleReacher", "LongSimpleReacher-v0": "LongSimpleReacher",
        "HoleReacher-v0": "HoleReacher"}


def spec_of(env):
    """oracle MPSpec from the resolved C config of a BlackBoxVectorEnv."""
    c = env._eng.cfg
    kind = {1: "promp", 2: "dmp", 3: "prodmp"}[c.mp_kind]
    return mp.MPSpec(kind=kind, dof=c.n_links, n_basis=c.n_basis, phase="linear" if c.phase_kind == 0 else "exp",
                     tau=c.tau, delay=c.delay, alpha_phase=c.alpha_phase, bandwidth=c.bandwidth,
                     zero_start=c.zero_start, zero_goal=c.zero_goal, basis_outside=c.num_basis_outside, weights_scale=c.weights_scale,
                     goal_scale=c.goal_scale, alpha=c.alpha, pc_length=c.pc_length, dt=c.dt, duration=c.duration,
                     basis_dt=c.basis_dt if c.mp_kind == 3 else 0.0)


def ctrl_of(env):
    c = env._eng.cfg
    if c.ctrl_kind == 0 and c.n_gains:   # per-joint gains (numpy arrays broadcast like the reference)
        return ("pd", np.array(c.p_gains[:c.n_gains]), np.array(c.d_gains[:c.n_gains]))
    return {0: ("pd", c.p_gain, c.d_gain), 1: ("vel",), 2: ("pos",)}[c.ctrl_kind]


def oracle_kwargs(env):
    c = env._eng.cfg
    return dict(replan_period=c.replan_period, condition_on_desired=bool(c.condition_on_desired),
                max_planning_times=c.max_planning_times if c.max_planning_times > 0 else np.inf)


def oracle_tables(spec, rows):
    t = mp.build_tables(spec, rows)
    if spec.kind == "prodmp":
        nb = spec.n_basis
        return np.concatenate([t["pb"], t["vb"], t["y1"][:, None], t["y2"][:, None], t["dy1"][:, None],
                               t["dy2"][:, None]], 1)
    key = "phi" if spec.kind == "promp" else "psi"
    last = "dt32" if spec.kind == "promp" else "sdt"
    return np.concatenate([t[key], t[last][:rows, None]], 1)


def oracle_tables_dict(spec, env):
    """The oracle's own tables (oracle/mp.py:build_tables) over the handle's row count: what every
    device-vs-oracle comparison uses (test_tables_bit_exact pins them equal to the device's)."""
    return mp.build_tables(spec, env._eng.dims.table_rows)


def split_tables(spec, arr):
    nb = spec.n_basis
    if spec.kind == "prodmp":
        return dict(pb=arr[:, :nb + 1], vb=arr[:, nb + 1:2 * nb + 2], y1=arr[:, 2 * nb + 2], y2=arr[:, 2 * nb + 3],
                    dy1=arr[:, 2 * nb + 4], dy2=arr[:, 2 * nb + 5])
    if spec.kind == "promp":
        return dict(phi=arr[:, :nb], dt32=arr[:, nb])
    return dict(psi=arr[:, :nb], sdt=arr[:, nb])


def assert_ulps(got, ref, max_ulps):
    """f64 arrays equal within max_ulps units in the last place (infinities must match)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(got[~fin], ref[~fin])
    ulps = np.abs(got[fin] - ref[fin]) / np.spacing(np.abs(ref[fin]))
    bad = np.nonzero(ulps > max_ulps)[0]
    assert bad.size == 0, (f"{bad.size} values beyond {max_ulps} ulp (max {ulps.max():.1f}): "
                           f"got={got[fin][bad][:4]}, ref={ref[fin][bad][:4]}")


def ulp_diff32(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# ------------------------------------------------------------------------------------ resets
@pytest.mark.parametrize("name", ["SimpleReacher-v0", "LongSimpleReacher-v0", "HoleReacher-v0"])
def test_reset_matches_numpy_streams(name):
    N = 300
    env = fgx.make(f"fancy_ProMP/{name}", num_envs=N, device=DEV)
    ob = batched.BatchedReacher(NAME[name], N)
    obs, _ = env.reset(seed=5)
    o_ref = ob.reset(list(range(N)), [5 + i for i in range(N)])
    for r in range(4):
        st = env.get_state()
        np.testing.assert_array_equal(np_(st["q"]), ob.q)
        np.testing.assert_array_equal(np_(st["qd"]), ob.qd)
        np.testing.assert_array_equal(np_(st["goal"]), ob.goal)
        if "Hole" in name:
            np.testing.assert_array_equal(np_(st["hole"])[:, 0], ob.hole_x)
            np.testing.assert_array_equal(np_(st["hole"])[:, 1], ob.hole_w)
        close(np_(obs), o_ref[:, ob.mask])
        obs, _ = env.reset()                     # unseeded: continue every env's PCG64 stream
        o_ref = ob.reset(list(range(N)))


def test_reset_golden():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "resets.npz"))
    for kind, name in (("simple", "SimpleReacher-v0"), ("long", "LongSimpleReacher-v0"), ("hole", "HoleReacher-v0")):
        env = fgx.make(f"fancy_ProDMP/{name}", num_envs=64, device=DEV)
        env.reset(seed=0)
        st = env.get_state()
        np.testing.assert_array_equal(np_(st["q"]), g[f"{kind}_q0"])
        np.testing.assert_array_equal(np_(st["goal"]), g[f"{kind}_goal"])
        for r in range(3):
            env.reset()
            st = env.get_state()
            np.testing.assert_array_equal(np_(st["q"]), g[f"{kind}_cont_q0"][:, r])
            np.testing.assert_array_equal(np_(st["goal"]), g[f"{kind}_cont_goal"][:, r])


# ------------------------------------------------------------------------------------ tables / MP
MP_IDS = ["fancy_ProMP/LongSimpleReacher-v0", "fancy_ProMP/SimpleReacher-v0", "fancy_DMP/LongSimpleReacher-v0",
          "fancy_DMP/SimpleReacher-v0", "fancy_ProDMP/HoleReacher-v0", "fancy_ProDMP/SimpleReacher-v0",
          "fancy_ProMP/HoleReacher-v0", "fancy_DMP/HoleReacher-v0"]


@pytest.mark.parametrize("env_id", MP_IDS)
def test_tables_bit_exact(env_id):
    """The device's basis tables equal the oracle's (oracle/mp.py:build_tables) bit for bit: both
    compute in f64 with the same exp (csrc/fgx_exp.h == oracle/mp.py:exp64) and round once to f32."""
    env = fgx.make(env_id, num_envs=8, device=DEV)
    spec = spec_of(env)
    got = np_(env.tables())
    ref = oracle_tables(spec, got.shape[0])
    got = got[:, :ref.shape[1]]
    d = ulp_diff32(got, ref)
    assert d.max() == 0, f"{int((d != 0).sum())} entries differ, max {d.max()} ulp"


@pytest.mark.parametrize("env_id", MP_IDS)
def test_trajectory_bit_exact(env_id):
    N = 333
    env = fgx.make(env_id, num_envs=N, device=DEV)
    env.reset(seed=11)
    spec = spec_of(env)
    tabs = oracle_tables_dict(spec, env)   # the oracle's own tables (== the device's, bit for bit)
    rng = np.random.default_rng(0)
    params = rng.standard_normal((N, env.n_params), dtype=np.float32)
    st = env.get_state()
    pos, vel = env.trajectory(torch.from_numpy(params).to(DEV))
    rp, rv = mp.trajectory(spec, tabs, params, 0, np_(st["q"]), np_(st["qd"]))
    np.testing.assert_array_equal(np_(pos), rp)
    np.testing.assert_array_equal(np_(vel), rv)


# ------------------------------------------------------------------------------------ BB given traj
GOLDEN_BB = {
    "bb_simple": "fancy_ProMP/SimpleReacher-v0",
    "bb_long": "fancy_ProMP/LongSimpleReacher-v0",
    "bb_hole_vel": "fancy_ProMP/HoleReacher-v0",
    "bb_hole_pd": "fancy_ProDMP/HoleReacher-v0",
    "bb_replan": "fancy_ProDMP/SimpleReacher-v0",
}


@pytest.mark.parametrize("case", list(GOLDEN_BB))
def test_bb_golden_given_trajectory(case):
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", case + ".npz"))
    E, n_bb = g["ret"].shape
    over = None
    if case == "bb_replan":
        over = {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(25)}}
    env = fgx.make(GOLDEN_BB[case], num_envs=E, device=DEV, mp_config_override=over, info_level=2)
    obs0, _ = env.reset(seed=[100 + i for i in range(E)])
    close(np_(obs0), g["obs0"])
    for b in range(n_bb):
        steps = np_(env.get_state()["steps"])
        P = np.stack([g["pos"][i, steps[i]:steps[i] + 200] for i in range(E)])
        V = np.stack([g["vel"][i, steps[i]:steps[i] + 200] for i in range(E)])
        obs, ret, te, tr, info = env.step_trajectory(torch.from_numpy(P), torch.from_numpy(V))
        tl = np_(info["trajectory_length"])
        np.testing.assert_array_equal(tl, g["tlen"][:, b])
        np.testing.assert_array_equal(np_(te), g["term"][:, b])
        np.testing.assert_array_equal(np_(tr), g["trunc"][:, b])
        close(np_(ret), g["ret"][:, b])
        close(np_(info["final_observation"]), g["obs"][:, b])
        for i in range(E):
            L = tl[i]
            close(np_(info["step_actions"])[i, :L], g["actions"][i, b, :L])
            close(np_(info["step_observations"])[i, :L], g["step_obs"][i, b, :L])
            close(np_(info["step_rewards"])[i, :L], g["step_rew"][i, b, :L])
        done = g["term"][:, b] | g["trunc"][:, b]
        close(np_(obs)[done], g["reset_obs"][:, b][done])


# ------------------------------------------------------------------------------------ full BB step
FULL = [
    ("fancy_ProMP/LongSimpleReacher-v0", None, 512, 3),
    ("fancy_ProMP/SimpleReacher-v0", None, 512, 2),
    ("fancy_DMP/LongSimpleReacher-v0", None, 512, 2),
    ("fancy_ProDMP/HoleReacher-v0", None, 512, 3),
    ("fancy_ProMP/HoleReacher-v0", None, 512, 3),
    ("fancy_DMP/HoleReacher-v0", None, 256, 2),
    ("fancy_ProDMP/SimpleReacher-v0", {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(25)}}, 256, 10),
    ("fancy_ProMP/HoleReacher-v0", {"controller_kwargs": {"controller_type": "position"}}, 256, 2),
    ("fancy_ProDMP/SimpleReacher-v0", {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(25),
                                                            "condition_on_desired": True}}, 256, 10),
    ("fancy_ProDMP/SimpleReacher-v0", {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(25),
                                                            "max_planning_times": 3}}, 128, 6),
    ("fancy_DMP/SimpleReacher-v0", {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(40)}}, 128, 6),
    ("fancy_ProMP/LongSimpleReacher-v0", {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(50)}}, 128, 5),
    ("fancy_ProDMP/HoleReacher-v0", {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(30)}}, 256, 8),
]


@pytest.mark.parametrize("ci", range(len(FULL)))
def test_bb_step_vs_oracle(ci):
    env_id, over, N, n_bb = FULL[ci]
    env = fgx.make(env_id, num_envs=N, device=DEV, mp_config_override=over, info_level=2)
    spec = spec_of(env)
    tabs = oracle_tables_dict(spec, env)   # the oracle's own tables (== the device's, bit for bit)
    name = NAME[env_id.split("/")[1]]
    ob = batched.BatchedBB(name, N, ctrl_of(env), mp_spec=spec, info_level=2, tables=tabs, **oracle_kwargs(env))
    o_g, _ = env.reset(seed=1000)
    o_r = ob.reset(seed=1000)
    close(np_(o_g), o_r)
    rng = np.random.default_rng(77)
    n_exact = 0
    for b in range(n_bb):
        params = rng.standard_normal((N, env.n_params), dtype=np.float32)
        obs, ret, te, tr, info = env.step(torch.from_numpy(params).to(DEV))
        r_obs, r_ret, r_te, r_tr, r_info = ob.step(params)
        np.testing.assert_array_equal(np_(info["trajectory_length"]), r_info["trajectory_length"])
        np.testing.assert_array_equal(np_(te), r_te)
        np.testing.assert_array_equal(np_(tr), r_tr)
        np.testing.assert_array_equal(np_(info["positions"]), r_info["positions"])
        np.testing.assert_array_equal(np_(info["velocities"]), r_info["velocities"])
        close(np_(ret), r_ret)
        # numpy's pairwise summation order is reproduced for every trajectory length
        # (np.linalg.norm / np.dot go through the host BLAS: the kernel follows the OpenBLAS
        # fma ordering pinned by the goldens; another host BLAS may round differently by an ulp)
        assert_ulps(np_(ret), r_ret, 16)
        n_exact += int((np_(ret) == r_ret).sum())
        close(np_(info["final_observation"]), r_info["final_obs"])
        close(np_(obs), r_obs)
        L = r_info["trajectory_length"]
        sa = np_(info["step_actions"])
        so = np_(info["step_observations"])
        sr = np_(info["step_rewards"])
        for i in range(0, N, 37):
            close(sa[i, :L[i]], r_info["step_actions"][i, :L[i]])
            close(so[i, :L[i]], r_info["step_observations"][i, :L[i]])
            close(sr[i, :L[i]], r_info["step_rewards"][i, :L[i]])
            if "is_collided" in info:
                np.testing.assert_array_equal(np_(info["is_collided"])[i, :L[i]].astype(bool),
                                              r_info["is_collided"][i, :L[i]])
                np.testing.assert_array_equal(np_(info["is_success"])[i, :L[i]].astype(bool),
                                              r_info["is_success"][i, :L[i]])
                close(np_(info["end_effector"])[i, :L[i]], r_info["end_effector"][i, :L[i]])
            else:
                close(np_(info["reward_dist"])[i, :L[i]], r_info["reward_dist"][i, :L[i]])
                close(np_(info["reward_ctrl"])[i, :L[i]], r_info["reward_ctrl"][i, :L[i]])
    assert n_exact >= 0.8 * N * n_bb, f"only {n_exact} returns bit-exact"


FAST = FULL + [
    ("fancy_DMP/SimpleReacher-v0", {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(40)}}, 256, 8),
    ("fancy_ProMP/LongSimpleReacher-v0", {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(64)}}, 192, 6),
    # segment lengths 150 / 50 and 170 / 30: the pairwise split (L/2) & ~7 != that of T = 200
    ("fancy_ProMP/LongSimpleReacher-v0", {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(150)}}, 128, 4),
    ("fancy_ProDMP/SimpleReacher-v0", {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(170)}}, 128, 4),
    # clip-free blocks (ProMP + PD): waves of unit-scale weights take them, waves with weights x300
    # (controls beyond +-1000, np.clip active) or mixed lanes take the clipping body
    ("fancy_ProMP/LongSimpleReacher-v0", None, 320, 3, "clipmix"),
    ("fancy_ProMP/SimpleReacher-v0", {"controller_kwargs": {"p_gains": 40.0, "d_gains": 3.0}}, 256, 3, "clipmix"),
]


def param_scale(kind, N):
    """per-env weight multipliers: wave 0 unit, wave 1 every 9th lane x300, wave 2 all x300,
    wave 3 x30 (near the clip-free bound), the rest unit"""
    s = np.ones(N, np.float32)
    if kind == "clipmix":
        s[64:128:9] = 300.0
        s[128:192] = 300.0
        s[192:256] = 30.0
    return s


@pytest.mark.parametrize("ci", range(len(FAST)))
def test_bb_fast_path_vs_oracle(ci, monkeypatch):
    """info_level 0 runs the unrolled fast loop (fgx_kernels.h k_episode): returns, flags, lengths,
    observations and the full f64 env state after every BB step.  After the first step every
    third env is reset (unseeded, reset_mask) so that lanes of one wave sit at different env
    steps and replanning phases, which the wave-uniform fast-block count must respect."""
    env_id, over, N, n_bb = FAST[ci][:4]
    scale = param_scale(FAST[ci][4] if len(FAST[ci]) > 4 else None, N)
    if len(FAST[ci]) > 4:
        monkeypatch.setenv("FGX_EPISODE_KERNEL", "classic")   # the clip-free blocks live in k_episode
    env = fgx.make(env_id, num_envs=N, device=DEV, mp_config_override=over, info_level=0)
    spec = spec_of(env)
    name = NAME[env_id.split("/")[1]]
    ob = batched.BatchedBB(name, N, ctrl_of(env), mp_spec=spec, info_level=0,
                           **oracle_kwargs(env))
    close(np_(env.reset(seed=2000)[0]), ob.reset(seed=2000))
    rng = np.random.default_rng(91)
    n_exact = 0
    for b in range(n_bb):
        params = rng.standard_normal((N, env.n_params), dtype=np.float32) * scale[:, None]
        obs, ret, te, tr, info = env.step(torch.from_numpy(params).to(DEV))
        r_obs, r_ret, r_te, r_tr, r_info = ob.step(params)
        np.testing.assert_array_equal(np_(info["trajectory_length"]), r_info["trajectory_length"])
        np.testing.assert_array_equal(np_(te), r_te)
        np.testing.assert_array_equal(np_(tr), r_tr)
        close(np_(ret), r_ret)
        assert_ulps(np_(ret), r_ret, 16)
        n_exact += int((np_(ret) == r_ret).sum())
        close(np_(info["final_observation"]), r_info["final_obs"])
        close(np_(obs), r_obs)
        st = env.get_state()
        np.testing.assert_array_equal(np_(st["q"]), ob.env.q)
        np.testing.assert_array_equal(np_(st["qd"]), np.asarray(ob.env.qd, np.float64))
        np.testing.assert_array_equal(np_(st["steps"]), ob.env.steps)
        if b == 0:
            mask = np.zeros(N, np.uint8)
            mask[::3] = 1
            o_g, _ = env.reset(options={"reset_mask": torch.from_numpy(mask)})
            o_r = ob._reset_idx([i for i in range(N) if mask[i]])
            close(np_(o_g)[mask == 1], o_r)
    assert n_exact >= 0.8 * N * n_bb, f"only {n_exact} returns bit-exact"


def test_step_based_golden():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "step_based.npz"))
    for kind, name in (("simple", "fancy/SimpleReacher-v0"), ("long", "fancy/LongSimpleReacher-v0"),
                       ("hole", "fancy/HoleReacher-v0")):
        acts = g[f"{kind}_actions"]
        E = acts.shape[1]
        env = fgx.make(name, num_envs=E, device=DEV)
        o0, _ = env.reset(seed=0)
        close(np_(o0), g[f"{kind}_obs0"])
        for t in range(acts.shape[0]):
            obs, rew, te, tr, info = env.step(torch.from_numpy(acts[t]))
            np.testing.assert_array_equal(np_(te), g[f"{kind}_term"][t])
            np.testing.assert_array_equal(np_(tr), g[f"{kind}_trunc"][t])
            close(np_(info["final_observation"]), g[f"{kind}_obs"][t])
            close(np_(rew), g[f"{kind}_rew"][t])
            done = g[f"{kind}_term"][t] | g[f"{kind}_trunc"][t]
            if done.any():
                close(np_(obs)[done], g[f"{kind}_reset_obs"][t][done])


def test_large_batch_invariants():
    """BASELINE metric size: properties that do not need the oracle."""
    N = 65536
    env = fgx.make("fancy_ProMP/LongSimpleReacher-v0", num_envs=N, device=DEV, info_level=0)
    env.reset(seed=0)
    params = torch.randn((N, env.n_params), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    obs, ret, te, tr, info = env.step(params)
    assert bool((info["trajectory_length"] == 200).all())
    assert bool(tr.all()) and not bool(te.any())
    assert bool(torch.isfinite(ret).all()) and bool((ret <= 0).all())
    # the same seed and params give the same result (determinism, test/utils.py:72-88)
    env2 = fgx.make("fancy_ProMP/LongSimpleReacher-v0", num_envs=N, device=DEV, info_level=0)
    env2.reset(seed=0)
    obs2, ret2, te2, tr2, _ = env2.step(params)
    assert torch.equal(ret, ret2) and torch.equal(obs, obs2)
    # spot-check 64 envs against the oracle
    idx = np.arange(0, N, N // 64)
    spec = spec_of(env)
    ob = batched.BatchedBB("LongSimpleReacher", len(idx), ctrl_of(env), mp_spec=spec,
                           )
    ob._reset_idx(list(range(len(idx))), [int(i) for i in idx])
    _, r_ret, _, _, r_info = ob.step(np_(params)[idx])
    close(np_(ret)[idx], r_ret)
    close(np_(info["final_observation"])[idx], r_info["final_obs"])


def test_reset_mask_and_determinism():
    N = 256
    env = fgx.make("fancy_ProMP/HoleReacher-v0", num_envs=N, device=DEV, info_level=0)
    env.reset(seed=9)
    before = {k: np_(v) for k, v in env.get_state().items()}
    mask = np.zeros(N, np.uint8)
    mask[::3] = 1
    env.reset(options={"reset_mask": torch.from_numpy(mask)})   # unseeded reset of a subset
    after = {k: np_(v) for k, v in env.get_state().items()}
    ob = batched.BatchedReacher("HoleReacher", N)
    ob.reset(list(range(N)), [9 + i for i in range(N)])
    ob.reset([i for i in range(N) if mask[i]])
    np.testing.assert_array_equal(after["q"], ob.q)
    np.testing.assert_array_equal(after["goal"], ob.goal)
    keep = mask == 0
    np.testing.assert_array_equal(after["q"][keep], before["q"][keep])


# ------------------------------------------------------------------------------------ basis counts
NB_CASES = [
    ("fancy_ProMP/LongSimpleReacher-v0", 3), ("fancy_ProMP/SimpleReacher-v0", 8),
    ("fancy_DMP/LongSimpleReacher-v0", 10), ("fancy_ProDMP/HoleReacher-v0", 4),
    ("fancy_ProDMP/SimpleReacher-v0", 12), ("fancy_ProMP/ViaPointReacher-v0", 7),
]


def test_per_joint_pd_gains():
    """PDController with one gain per joint (tuple gains broadcast against the joint arrays)."""
    over = {"controller_kwargs": {"p_gains": (0.5, 0.9, 1.3, 0.7, 2.0), "d_gains": [0.05, 0.1, 0.2, 0.02, 0.3]}}
    N = 256
    env = fgx.make("fancy_ProMP/LongSimpleReacher-v0", num_envs=N, device=DEV, info_level=0, mp_config_override=over)
    spec = spec_of(env)
    ob = batched.BatchedBB("LongSimpleReacher", N, ctrl_of(env), mp_spec=spec,
                           **oracle_kwargs(env))
    assert ctrl_of(env)[1].shape == (5,)
    close(np_(env.reset(seed=8)[0]), ob.reset(seed=8))
    rng = np.random.default_rng(1)
    for b in range(2):
        params = rng.standard_normal((N, env.n_params), dtype=np.float32)
        obs, ret, te, tr, info = env.step(torch.from_numpy(params).to(DEV))
        r_obs, r_ret, r_te, r_tr, r_info = ob.step(params)
        assert_ulps(np_(ret), r_ret, 16)
        close(np_(obs), r_obs)
        np.testing.assert_array_equal(np_(env.get_state()["q"]), ob.env.q)


@pytest.mark.parametrize("ci", range(len(NB_CASES)))
def test_generic_basis_count(ci):
    """num_basis != 5 (mp_config_override basis_generator_kwargs) runs the generic NB
    instantiation: trajectories bit-exact given the tables, BB steps vs the oracle."""
    env_id, nb = NB_CASES[ci]
    over = {"basis_generator_kwargs": {"num_basis": nb}}
    N = 192
    env = fgx.make(env_id, num_envs=N, device=DEV, info_level=0, mp_config_override=over)
    spec = spec_of(env)
    assert spec.n_basis == nb and env.n_params == spec.n_params
    tabs = oracle_tables_dict(spec, env)   # the oracle's own tables (== the device's, bit for bit)
    ref_t = oracle_tables(spec, np_(env.tables()).shape[0])
    assert ulp_diff32(np_(env.tables())[:, :ref_t.shape[1]], ref_t).max() <= 1
    env.reset(seed=4)
    rng = np.random.default_rng(6)
    params = rng.standard_normal((N, env.n_params), dtype=np.float32)
    st = env.get_state()
    pos, vel = env.trajectory(torch.from_numpy(params).to(DEV))
    rp, rv = mp.trajectory(spec, tabs, params, 0, np_(st["q"]), np_(st["qd"]))
    np.testing.assert_array_equal(np_(pos), rp)
    np.testing.assert_array_equal(np_(vel), rv)
    name = env_id.split("/")[1].replace("-v0", "")
    ob = batched.BatchedBB(name, N, ctrl_of(env), mp_spec=spec, tables=tabs, **oracle_kwargs(env))
    close(np_(env.reset(seed=4)[0]), ob.reset(seed=4))
    for b in range(2):
        params = rng.standard_normal((N, env.n_params), dtype=np.float32)
        obs, ret, te, tr, info = env.step(torch.from_numpy(params).to(DEV))
        r_obs, r_ret, r_te, r_tr, r_info = ob.step(params)
        np.testing.assert_array_equal(np_(info["trajectory_length"]), r_info["trajectory_length"])
        np.testing.assert_array_equal(np_(te), r_te)
        assert_ulps(np_(ret), r_ret, 16)
        close(np_(obs), r_obs)
        np.testing.assert_array_equal(np_(env.get_state()["q"]), ob.env.q)


@pytest.mark.parametrize("name,kw", [("HoleReacher", {}), ("HoleReacher", {"hole_width": 0.3, "hole_x": 1.0}),
                                     ("HoleReacher", {"rew_fct": "unbounded"})])
def test_wall_collision_randomised_raw_steps(name, kw):
    """Many random arm configurations through the step-based env: the device wall check (binary
    searches over the monotone link points, fgx_device.h wall_collision) must flag exactly the
    states the reference's 100-points-per-link test flags."""
    N, steps = 2048, 60
    env = fgx.make("fancy/HoleReacher-v0", num_envs=N, device=DEV, **kw)
    env.reset(seed=123)
    ob = batched.BatchedReacher(name, N, **kw)
    ob.reset(list(range(N)), [123 + i for i in range(N)])
    rng = np.random.default_rng(31)
    drift = rng.uniform(-3.0, 3.0, (N, 5))
    n_coll = 0
    for t in range(steps):
        a = (rng.uniform(-np.pi, np.pi, (N, 5)) + drift).astype(np.float32)
        obs, rew, te, tr, info = env.step(torch.from_numpy(a))
        o_r, r_r, te_r, tr_r, _ = ob.step(a.astype(np.float64), np.ones(N, bool), True)
        np.testing.assert_array_equal(np_(te).astype(bool), te_r)
        np.testing.assert_array_equal(np_(tr).astype(bool), tr_r)
        close(np_(rew), r_r)
        close(np_(info["final_observation"]), o_r)
        n_coll += int(te_r.sum())
        done = np.nonzero(te_r | tr_r)[0]
        if len(done):
            ob.reset(list(done))
    assert n_coll > 100


@pytest.mark.parametrize("name,N", [("SimpleReacher", 1000), ("LongSimpleReacher", 257), ("HoleReacher", 513)])
def test_step_raw_ragged_vs_oracle(name, N):
    """k_step_raw stages each workgroup's action / observation rows through LDS: env counts that
    leave a partial last workgroup (1000 = 3·256 + 232, 257, 513), 205 steps so the TimeLimit
    truncates and auto-resets every env once; final and reset observations, rewards, flags
    and the whole f64 state vs the oracle."""
    env = fgx.make(f"fancy/{name}-v0", num_envs=N, device=DEV)
    o0, _ = env.reset(seed=5)
    ob = batched.BatchedReacher(name, N)
    close(np_(o0), ob.reset(list(range(N)), [5 + i for i in range(N)]))
    rng = np.random.default_rng(8)
    n = env.dof
    for t in range(205):
        a = rng.uniform(-20.0, 20.0, (N, n)).astype(np.float32)
        obs, rew, te, tr, info = env.step(torch.from_numpy(a))
        o_r, r_r, te_r, tr_r, _ = ob.step(a.astype(np.float64), np.ones(N, bool), True)
        np.testing.assert_array_equal(np_(te).astype(bool), te_r)
        np.testing.assert_array_equal(np_(tr).astype(bool), tr_r)
        close(np_(rew), r_r)
        close(np_(info["final_observation"]), o_r)
        done = np.nonzero(te_r | tr_r)[0]
        if len(done):
            close(np_(obs)[done], ob.reset(list(done)))
        if t % 50 == 0 or t == 204:
            st = env.get_state()
            np.testing.assert_array_equal(np_(st["q"]), ob.q)
            np.testing.assert_array_equal(np_(st["qd"]), np.asarray(ob.qd, np.float64))
            np.testing.assert_array_equal(np_(st["steps"]), ob.steps)


def test_set_state_then_step_matches_oracle():
    """fgx_set_state (checkpoint restore): a BB step from an arbitrary restored state."""
    N = 192
    env = fgx.make("fancy_ProDMP/HoleReacher-v0", num_envs=N, device=DEV, info_level=0)
    env.reset(seed=17)
    rng = np.random.default_rng(2)
    st = {k: np_(v) for k, v in env.get_state().items()}
    q = st["q"] + rng.uniform(-0.3, 0.3, st["q"].shape)
    qd = rng.uniform(-1, 1, st["qd"].shape)
    steps = rng.integers(0, 150, N).astype(np.int32)
    env.set_state(q=q, qd=qd, steps=steps)
    back = {k: np_(v) for k, v in env.get_state().items()}
    np.testing.assert_array_equal(back["q"], q)
    np.testing.assert_array_equal(back["qd"], qd)
    np.testing.assert_array_equal(back["steps"], steps)
    spec = spec_of(env)
    ob = batched.BatchedBB("HoleReacher", N, ctrl_of(env), mp_spec=spec,
                           **oracle_kwargs(env))
    ob.reset(seed=17)
    ob.env.q, ob.env.qd, ob.env.steps = q.copy(), qd.copy(), steps.astype(np.int64)
    ob.env._fk()
    params = rng.standard_normal((N, env.n_params), dtype=np.float32)
    obs, ret, te, tr, info = env.step(torch.from_numpy(params).to(DEV))
    r_obs, r_ret, r_te, r_tr, r_info = ob.step(params)
    np.testing.assert_array_equal(np_(info["trajectory_length"]), r_info["trajectory_length"])
    np.testing.assert_array_equal(np_(te), r_te)
    np.testing.assert_array_equal(np_(tr), r_tr)
    assert_ulps(np_(ret), r_ret, 16)
    close(np_(obs), r_obs)


def test_no_autoreset_and_mean_aggregation():
    """autoreset=False keeps finished envs (gymnasium without the VectorEnv wrapper);
    reward_aggregation=np.mean divides the pairwise sum by the trajectory length."""
    N = 128
    over = {"black_box_kwargs": {"reward_aggregation": np.mean}}
    env = fgx.make("fancy_ProMP/SimpleReacher-v0", num_envs=N, device=DEV, info_level=0, autoreset=False,
                   mp_config_override=over)
    ref = fgx.make("fancy_ProMP/SimpleReacher-v0", num_envs=N, device=DEV, info_level=0)
    env.reset(seed=5)
    ref.reset(seed=5)
    params = torch.from_numpy(np.random.default_rng(0).standard_normal((N, env.n_params), dtype=np.float32)).to(DEV)
    obs, ret, te, tr, info = env.step(params)
    obs_r, ret_r, te_r, tr_r, info_r = ref.step(params)
    assert bool(tr.all())
    np.testing.assert_array_equal(np_(obs), np_(info_r["final_observation"]))   # not reset
    np.testing.assert_array_equal(np_(ret), np_(ret_r) / np_(info_r["trajectory_length"]).astype(np.float64))
    assert bool((env.get_state()["steps"] == 200).all())
    obs2, ret2, te2, tr2, info2 = env.step(params)   # past the TimeLimit: truncated after 1 step
    assert bool((info2["trajectory_length"] == 1).all()) and bool(tr2.all())


def test_step_before_reset_raises():
    """gymnasium's OrderEnforcing: step() before reset() raises ResetNeeded."""
    env = fgx.make("fancy_ProMP/SimpleReacher-v0", num_envs=8, device=DEV)
    with pytest.raises(fgx.ResetNeeded):
        env.step(torch.zeros((8, env.n_params)))
    env.reset(seed=0)
    env.step(torch.zeros((8, env.n_params)))
    raw = fgx.make("fancy/SimpleReacher-v0", num_envs=8, device=DEV)
    with pytest.raises(fgx.ResetNeeded):
        raw.step(torch.zeros((8, 2)))


@pytest.mark.parametrize("env_id,N", [("fancy_ProMP/LongSimpleReacher-v0", 4099), ("fancy_ProDMP/HoleReacher-v0", 4099),
                                      ("fancy_ProMP/SimpleReacher-v0", 1000), ("fancy_ProDMP/SimpleReacher-v0", 65536)])
def test_trajectory_mfma_equals_valu(env_id, N, monkeypatch):
    """k_traj_mfma (csrc/fgx_mfma.h: ProMP positions once, forward differences across the half-waves,
    8-row LDS groups) against k_traj_valu on the same plans (a replanning schedule that never fires
    before T routes get_trajectory to the VALU kernel) and against round 3's k_traj_mfma_r3
    (FGX_TRAJ_R3): bit for bit, partial last wave included."""
    outs = []
    for over, r3 in ((None, False), ({"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(200)}}, False),
                     (None, True)):
        if r3:
            monkeypatch.setenv("FGX_TRAJ_R3", "1")
        env = fgx.make(env_id, num_envs=N, device=DEV, mp_config_override=over)
        params = torch.from_numpy(np.random.default_rng(5).standard_normal((N, env.n_params), dtype=np.float32)).to(DEV)
        env.reset(seed=3)
        outs.append([np_(x) for x in env.trajectory(params)])
    for other in (outs[1], outs[2]):
        for a, b in zip(outs[0], other):
            assert a.shape == b.shape
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("env_id,N,duration", [("fancy_ProMP/SimpleReacher-v0", 1000, 2.56),
                                               ("fancy_ProDMP/SimpleReacher-v0", 777, 2.56),
                                               ("fancy_ProMP/SimpleReacher-v0", 96, 2.28),
                                               ("fancy_ProDMP/SimpleReacher-v0", 64, 2.4)])
def test_trajectory_mfma_long_plans(env_id, N, duration, monkeypatch):
    """k_traj_mfma at the engine's longest plans (T <= 256): ProMP T = 256 is 9 tiles, two segments of
    the workgroup's 8 waves; T = 228 one segment whose last tile outputs 32 rows; ProDMP T = 256 / 240
    8 tiles.  Against k_traj_valu, bit for bit."""
    outs = []
    for replan in (None, int(round(duration / 0.01))):
        over = {"black_box_kwargs": {"duration": duration}}
        if replan:
            over["black_box_kwargs"]["replanning_schedule"] = fgx.ReplanEvery(replan)
        env = fgx.make(env_id, num_envs=N, device=DEV, mp_config_override=over)
        assert env.T == int(round(duration / 0.01))
        params = torch.from_numpy(np.random.default_rng(9).standard_normal((N, env.n_params), dtype=np.float32)).to(DEV)
        env.reset(seed=3)
        outs.append([np_(x) for x in env.trajectory(params)])
    for a, b in zip(outs[0], outs[1]):
        assert a.shape == b.shape
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("env_id,over", [
    ("fancy_ProDMP/HoleReacher-v0", {"basis_generator_kwargs": {"dt": 0.005}}),
    ("fancy_ProDMP/SimpleReacher-v0", {"basis_generator_kwargs": {"dt": 0.02}}),
    ("fancy_ProDMP/LongSimpleReacher-v0", {"basis_generator_kwargs": {"dt": 0.0075},
                                           "phase_generator_kwargs": {"delay": 0.2}}),
    ("fancy_ProMP/LongSimpleReacher-v0", {"phase_generator_kwargs": {"delay": -0.25}}),   # negative delay: ProMP
    ("fancy_DMP/SimpleReacher-v0", {"phase_generator_kwargs": {"delay": -0.1}}),          # and DMP accept it
])
def test_basis_dt_and_negative_delay_vs_oracle(env_id, over):
    """A ProDMP basis generator dt of its own (basis_generator_factory.py:8-23; its precompute grid,
    looked up at the rounded grid index of each env step) and a negative phase delay for ProMP / DMP
    (the phase clips max((t - delay) / tau, 0); fgx_create refuses a negative delay only for ProDMP):
    tables bit-exact, then BB steps end to end against the oracle."""
    N = 256
    env = fgx.make(env_id, num_envs=N, device=DEV, mp_config_override=over, info_level=0)
    spec = spec_of(env)
    got = np_(env.tables())
    ref = oracle_tables(spec, got.shape[0])
    np.testing.assert_array_equal(got[:, :ref.shape[1]].view(np.uint32), ref.view(np.uint32))
    ob = batched.BatchedBB(NAME[env_id.split("/")[1]], N, ctrl_of(env), mp_spec=spec, **oracle_kwargs(env))
    close(np_(env.reset(seed=4)[0]), ob.reset(seed=4))
    rng = np.random.default_rng(9)
    for _ in range(2):
        params = rng.standard_normal((N, env.n_params), dtype=np.float32)
        obs, ret, te, tr, info = env.step(torch.from_numpy(params).to(DEV))
        r_obs, r_ret, r_te, r_tr, r_info = ob.step(params)
        np.testing.assert_array_equal(np_(info["trajectory_length"]), r_info["trajectory_length"])
        np.testing.assert_array_equal(np_(te).astype(bool), r_te)
        np.testing.assert_array_equal(np_(tr).astype(bool), r_tr)
        assert_ulps(np_(ret), r_ret, 16)
        close(np_(obs), r_obs)
        np.testing.assert_array_equal(np_(env.get_state()["q"]), ob.env.q)
    with pytest.raises(ValueError):   # ProDMP keeps refusing a negative delay
        fgx.make("fancy_ProDMP/SimpleReacher-v0", num_envs=8, device=DEV,
                 mp_config_override={"phase_generator_kwargs": {"delay": -0.1}})
