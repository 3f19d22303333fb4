"""Black-box candidate rollouts (fgx_kernels.h: k_rollout_bb; fgx_rollout_bb; BlackBoxVectorEnv.rollout):
the black-box step of C parameter vectors per env in one launch, from each env's current state, with
the handle left untouched.

The yardstick is the existing step path: a twin env built with autoreset=False, loaded with the env's
state_dict() and stepped once per candidate; every output is compared bit for bit (NaNs canonicalised,
test_gpu_wide._bits).  Every case runs at the registered T = 200 (the test-only 252-step id: T = 252) at
N = 200 (one partial workgroup per candidate) and N = 300 (a full and a partial one, the last wave
partial) with C in {1, 3}.  One section
compares with the CPU oracle instead, independently of the device's own step path."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import fancy_gym_crowd_amd as fgx
from fancy_gym_crowd_amd import _lib, registry
from fancy_gym_crowd_amd.vector_env import ResetNeeded
from oracle import batched
from test_gpu_parity import assert_ulps, close, ctrl_of, np_, oracle_kwargs, spec_of
from test_gpu_wide import _bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = "fgxrbb"
_REG = (registry.ENV_SPECS, registry._BB_IDS, registry.ALL_MOVEMENT_PRIMITIVE_ENVIRONMENTS,
        registry.MOVEMENT_PRIMITIVE_ENVIRONMENTS_FOR_NS)


@pytest.fixture(scope="module", autouse=True)
def long_id():
    """fgxrbb252/LongSimpleReacher-v0: the registered spec with max_episode_steps = 252 (the plan then
    lasts 252 samples: numpy's two-level sum, step rewards in the workspace on SimpleReacher); this module only."""
    saved = [copy.deepcopy(d) for d in _REG]
    base = registry.ENV_SPECS["fancy/LongSimpleReacher-v0"]
    fgx.register(f"{NS}252/LongSimpleReacher-v0", base.kind, base.kwargs, max_episode_steps=252, mp_config=base.mp_config)
    yield
    for d, s in zip(_REG, saved):
        d.clear()
        d.update(s)


def _bb(**kw):
    return {"black_box_kwargs": kw}


# name: (env id, mp_config_override, make kwargs, BB steps taken before the rollout, those steps auto-reset,
#        scale of the N(0, 1) parameters, "some but not all envs end early")
CONFIGS = {
    "promp_long": ("fancy_ProMP/LongSimpleReacher-v0", None, {}, 0, False, 1.0, False),
    "promp_long_x300": ("fancy_ProMP/LongSimpleReacher-v0", None, {}, 0, False, 300.0, False),
    "dmp_hole": ("fancy_DMP/HoleReacher-v0", None, {}, 0, False, 1.0, True),
    "prodmp_hole": ("fancy_ProDMP/HoleReacher-v0", None, {}, 0, False, 1.0, True),
    "promp_via": ("fancy_ProMP/ViaPointReacher-v0", None, {}, 0, False, 1.0, False),
    "prodmp_simple_replan25": ("fancy_ProDMP/SimpleReacher-v0", _bb(replanning_schedule=fgx.ReplanEvery(25)), {}, 3,
                               False, 1.0, False),
    # (N(0, 10) parameters: on the CPU oracle 28 of 300 envs have collided and been reset after three
    # steps, N(0, 1) plans replanned every 25 steps never collide: steps 0 / 25 / 50 / 75, plans 0 .. 3)
    "prodmp_hole_replan25": ("fancy_ProDMP/HoleReacher-v0", _bb(replanning_schedule=fgx.ReplanEvery(25)), {}, 3, True,
                             10.0, False),
    "promp_hole_normperiod": ("fancy_ProMP/HoleReacher-v0",
                              _bb(replanning_schedule=fgx.ReplanEvery(40) | fgx.ReplanNormPeriod(16, 18, 30.0)), {}, 2,
                              True, 1.0, False),
    "prodmp_simple_cond": ("fancy_ProDMP/SimpleReacher-v0",
                           _bb(replanning_schedule=fgx.ReplanEvery(25), max_planning_times=3, condition_on_desired=True),
                           {}, 2, False, 1.0, False),
    "prodmp_hole_pos": ("fancy_ProDMP/HoleReacher-v0", {"controller_kwargs": {"controller_type": "position"}}, {}, 0,
                        False, 1.0, False),
    "promp_hole_3links": ("fancy_ProMP/HoleReacher-v0", None, {"n_links": 3}, 0, False, 1.0, False),
    "promp_simple_8links": ("fancy_ProMP/SimpleReacher-v0", None, {"n_links": 8}, 0, False, 1.0, False),
    "promp_long_m252": (f"{NS}252_ProMP/LongSimpleReacher-v0", None, {}, 0, False, 1.0, False),
}


def _make(name, N, autoreset):
    env_id, over, kw = CONFIGS[name][:3]
    return fgx.make(env_id, num_envs=N, device=DEV, mp_config_override=over, info_level=0, autoreset=autoreset, **kw)


def _start(name, N, seed=21):
    """The env under test in the state the case asks for, and its twin (autoreset off)."""
    pre, auto, scale = CONFIGS[name][3:6]
    env = _make(name, N, auto)
    twin = _make(name, N, False)
    env.reset(seed=seed)
    g = torch.Generator().manual_seed(seed)
    for _ in range(pre):
        env.step((torch.randn(N, env.n_params, generator=g) * scale).to(DEV))
    return env, twin


def _params(name, env, C, seed=5):
    p = np.random.default_rng(seed).standard_normal((C, env.num_envs, env.n_params)).astype(np.float32)
    return p * np.float32(CONFIGS[name][5])


def _step_path(env, twin, params):
    """What the rollout must give: per candidate the twin loaded with env's state and stepped once."""
    sd = env.state_dict()
    out = {k: [] for k in ("returns", "lengths", "terminated", "truncated", "observations")}
    for c in range(params.shape[0]):
        twin.load_state_dict(sd)
        obs, ret, te, tr, info = twin.step(torch.from_numpy(params[c]).to(DEV))
        for k, v in zip(out, (ret, info["trajectory_length"], te, tr, obs)):
            out[k].append(np_(v))
    return {k: np.stack(v) for k, v in out.items()}


def _same(got, want, what=""):
    got = dict(zip(("returns", "lengths", "terminated", "truncated", "observations"), got))
    for k, w in want.items():
        g = np_(got[k])
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}{k}: {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        bad = np.nonzero((_bits(g).reshape(g.size, -1) != _bits(w).reshape(w.size, -1)).any(axis=1))[0]
        assert bad.size == 0, (f"{what}{k} differs at {bad.size} of {g.size} entries, first "
                               f"{np.unravel_index(bad[0], g.shape)}: {g.flat[bad[0]]!r} vs {w.flat[bad[0]]!r}")


# ------------------------------------------------------------------------------------ 1. the step path's bits
@pytest.mark.parametrize("shape", [(200, 3), (300, 1), (300, 3)], ids=lambda s: "N%d-C%d" % s)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_rollout_equals_step_path(name, shape):
    N, C = shape
    env, twin = _start(name, N)
    p = _params(name, env, C)
    want = _step_path(env, twin, p)
    got = env.rollout(torch.from_numpy(p).to(DEV))
    assert got[2].dtype == torch.bool and got[3].dtype == torch.bool
    L = want["lengths"]
    st = np_(env.get_state()["steps"])
    print(f"{name} {shape}: env steps {st.min()}..{st.max()}, lengths {L.min()}..{L.max()}, terminated "
          f"{int(want['terminated'].sum())}, truncated {int(want['truncated'].sum())} of {L.size} pairs")
    _same(got, want)
    pre, auto = CONFIGS[name][3:5]
    if CONFIGS[name][6]:   # some but not all envs end early, per candidate
        early = (L < env.T).sum(axis=1)
        assert ((0 < early) & (early < N)).all(), early
    if pre and not auto:
        assert (st > 0).all()   # the plan start row is not 0
    if pre and auto:
        assert len(set(st.tolist())) > 1   # envs sit at different step counts
    if name == "promp_via":
        assert np.isneginf(want["returns"]).any()
    if name == "promp_long_m252":
        assert env.T == 252 and env._eng.cfg.max_episode_steps == 252 and (L == 252).all()


def test_long_segment_uses_the_workspace():
    """max_episode_steps = 252 (the plan lasts 252 samples too): SimpleReacher segments of 252 samples,
    summed from the step rewards in the caller's workspace, [C][T][N] doubles, in numpy's two-level order."""
    N, C = 200, 3
    env, twin = _start("promp_long_m252", N, seed=4)
    assert env.T == 252
    n = ctypes.c_int64()
    _lib.check(env._eng.lib.fgx_rollout_bb_workspace(env._eng.h, C, ctypes.byref(n)))
    assert n.value == 8 * C * 252 * N
    p = np.random.default_rng(8).standard_normal((C, N, env.n_params)).astype(np.float32)
    want = _step_path(env, twin, p)
    assert (want["lengths"] == 252).all()
    _same(env.rollout(torch.from_numpy(p).to(DEV)), want)


# ------------------------------------------------------------------------------------ 2. nothing changes
@pytest.mark.parametrize("name", ["promp_long", "prodmp_hole_replan25", "prodmp_simple_cond"])
def test_rollout_leaves_the_handle_untouched(name):
    N, C = 300, 3
    env, twin = _start(name, N)
    before = env.state_dict()["blob"].clone()
    env.rollout(torch.from_numpy(_params(name, env, C)).to(DEV))
    after = env.state_dict()["blob"]
    assert torch.equal(before.view(torch.uint8), after.view(torch.uint8))
    # and the step that follows is the twin's step from the same state
    twin.load_state_dict(env.state_dict())
    twin.autoreset = env.autoreset
    p = torch.from_numpy(_params(name, env, 1, seed=6)[0]).to(DEV)
    a, b = env.step(p), twin.step(p)
    for x, y, k in zip(a[:4], b[:4], ("obs", "ret", "terminated", "truncated")):
        assert np.array_equal(_bits(np_(x)), _bits(np_(y))), k
    assert torch.equal(a[4]["trajectory_length"], b[4]["trajectory_length"])
    assert torch.equal(env.state_dict()["blob"].view(torch.uint8), twin.state_dict()["blob"].view(torch.uint8))


# ------------------------------------------------------------------------------------ 3. non-finite parameters
@pytest.mark.parametrize("name", ["promp_long", "prodmp_hole"])
def test_non_finite_parameters(name):
    N, C = 300, 3
    env, twin = _start(name, N)
    clean = _params(name, env, C)
    p = clean.copy()
    p[0, 7, 0] = np.nan          # a lane of a full wave (its wave leaves the fast blocks)
    p[1, 70, 3] = np.inf
    p[1, 299, 1] = -np.inf       # the partial last wave
    p[2, 130, :] = np.nan
    hit = np.zeros((C, N), bool)
    hit[0, 7] = hit[1, 70] = hit[1, 299] = hit[2, 130] = True
    want = _step_path(env, twin, p)
    want_clean = _step_path(env, twin, clean)
    got = env.rollout(torch.from_numpy(p).to(DEV))
    _same(got, want)
    # the other pairs are what they are without the non-finite rows
    for k, g in zip(want_clean, got):
        g, w = np_(g), want_clean[k]
        assert np.array_equal(_bits(g[~hit]), _bits(w[~hit])), k
    assert not np.isfinite(np_(got[0])[hit]).all()


# ------------------------------------------------------------------------------------ 4. the CPU oracle
@pytest.mark.parametrize("env_id", ["fancy_ProMP/LongSimpleReacher-v0", "fancy_ProDMP/HoleReacher-v0"])
def test_rollout_vs_oracle(env_id):
    N, C = 128, 2
    env = fgx.make(env_id, num_envs=N, device=DEV, info_level=0)
    ob = batched.BatchedBB(env_id.split("/")[1][:-3], N, ctrl_of(env), mp_spec=spec_of(env), **oracle_kwargs(env))
    close(np_(env.reset(seed=9)[0]), ob.reset(seed=9))
    p = np.random.default_rng(31).standard_normal((C, N, env.n_params)).astype(np.float32)
    ret, length, te, tr, obs = env.rollout(torch.from_numpy(p).to(DEV))
    for c in range(C):
        o = copy.deepcopy(ob)
        _, r_ret, r_te, r_tr, r_info = o.step(p[c])
        np.testing.assert_array_equal(np_(length[c]), r_info["trajectory_length"])
        np.testing.assert_array_equal(np_(te[c]), r_te)
        np.testing.assert_array_equal(np_(tr[c]), r_tr)
        assert_ulps(np_(ret[c]), r_ret, 16)
        close(np_(obs[c]), r_info["final_obs"])   # the observation before the oracle's auto-reset
        if "Hole" in env_id:
            assert 0 < r_te.sum() < N


# ------------------------------------------------------------------------------------ 5. graph capture
def test_rollout_in_a_graph():
    name, N, C = "prodmp_hole", 200, 3
    env, twin = _start(name, N)
    p = torch.from_numpy(_params(name, env, C)).to(DEV)
    env.rollout(p)   # (the workspace of this C is allocated outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = env.rollout(p)
    torch.cuda.current_stream().wait_stream(side)
    for i in range(2):
        env.step(torch.from_numpy(_params(name, env, 1, seed=40 + i)[0]).to(DEV))   # the state moves on
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        eager = env.rollout(p)
        for a, b in zip(out, eager):
            assert np.array_equal(_bits(np_(a)), _bits(np_(b))), f"replay {i}"


def test_first_rollout_inside_a_capture_is_refused():
    env, _ = _start("prodmp_hole", 64)
    p = torch.from_numpy(_params("prodmp_hole", env, 2)).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with pytest.raises(RuntimeError, match="workspace"):
            with torch.cuda.graph(g, stream=side):
                env.rollout(p)
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------ 6. refusals and shapes
def _raw(env, p, C, ws=None, nbytes=0):
    N = env.num_envs
    ret = torch.empty((max(C, 1), N), dtype=torch.float64, device=DEV)
    ln = torch.empty((max(C, 1), N), dtype=torch.int32, device=DEV)
    te = torch.empty((max(C, 1), N), dtype=torch.uint8, device=DEV)
    tr = torch.empty_like(te)
    return env._eng.lib.fgx_rollout_bb(env._eng.h, ctypes.c_void_p(p.data_ptr()), C, ctypes.c_void_p(ret.data_ptr()),
                                       ctypes.c_void_p(ln.data_ptr()), ctypes.c_void_p(te.data_ptr()),
                                       ctypes.c_void_p(tr.data_ptr()), None,
                                       ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, nbytes,
                                       env._eng.stream())


def test_refusals_and_shapes():
    N = 64
    env = _make("prodmp_hole", N, False)
    p = torch.zeros((2, N, env.n_params), device=DEV)
    with pytest.raises(ResetNeeded):
        env.rollout(p)
    env.reset(seed=1)
    for bad in (torch.zeros((2, N + 1, env.n_params)), torch.zeros((2, N, env.n_params + 1)),
                torch.zeros((env.n_params,)), torch.zeros((1, 2, N, env.n_params)), torch.zeros((0, N, env.n_params))):
        with pytest.raises(ValueError, match="params"):
            env.rollout(bad)
    lib = env._eng.lib
    assert _raw(env, p, 0) == -1 and b"n_cand" in lib.fgx_last_error()
    n = ctypes.c_int64()
    _lib.check(lib.fgx_rollout_bb_workspace(env._eng.h, 2, ctypes.byref(n)))
    assert n.value == 8 * 2 * env.T * N   # a direct env at T = 200 > 128
    ws = torch.empty(n.value // 8, dtype=torch.float64, device=DEV)
    assert _raw(env, p, 2, ws, n.value - 8) == -1 and b"workspace" in lib.fgx_last_error()
    assert _raw(env, p, 2, None, 0) == -1 and b"workspace" in lib.fgx_last_error()
    assert _raw(env, p, 2, ws, n.value) == 0
    # SimpleReacher at the registered lengths needs none
    simple = _make("promp_long", N, False)
    _lib.check(lib.fgx_rollout_bb_workspace(simple._eng.h, 5, ctypes.byref(n)))
    assert n.value == 0

    def refused(word, env_id, over=None, **kw):
        e = fgx.make(env_id, num_envs=8, device=DEV, mp_config_override=over, info_level=0, **kw)
        e.reset(seed=0)
        with pytest.raises(ValueError, match=word):
            e.rollout(torch.zeros((2, 8, e.n_params), device=DEV))

    refused("learn", "fancy_ProMP/LongSimpleReacher-v0", {"phase_generator_kwargs": {"learn_tau": True}})
    refused("wide", "fancy_ProMP/LongSimpleReacher-v0", {"basis_generator_kwargs": {"num_basis": 13}})
    refused("validity", "fancy_ProMP/LongSimpleReacher-v0",
            traj_validity=fgx.TrajValidity(pos_low=[-1.2] * 5, pos_high=[1.2] * 5))
    refused("reward_aggregation", "fancy_ProMP/LongSimpleReacher-v0", _bb(reward_aggregation=np.max))


def test_two_dimensional_params_and_mean():
    name, N = "prodmp_hole", 200
    env, _ = _start(name, N)
    p = torch.from_numpy(_params(name, env, 1)).to(DEV)
    one = env.rollout(p)
    flat = env.rollout(p[0])
    assert tuple(flat[0].shape) == (N,) and tuple(flat[4].shape) == (N, env.out_dim)
    for a, b in zip(one, flat):
        assert np.array_equal(_bits(np_(a[0])), _bits(np_(b)))
    assert env.rollout(p, observations=False)[4] is None
    # np.mean: the step path's division of the same sum
    over = _bb(reward_aggregation=np.mean)
    em = fgx.make(CONFIGS[name][0], num_envs=N, device=DEV, mp_config_override=over, info_level=0, autoreset=False)
    tm = fgx.make(CONFIGS[name][0], num_envs=N, device=DEV, mp_config_override=over, info_level=0, autoreset=False)
    em.reset(seed=21)
    _same(em.rollout(p), _step_path(em, tm, np_(p)))
