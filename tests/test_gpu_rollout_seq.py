"""Black-box sequence rollouts (fgx_kernels.h: k_rollout_seq; fgx_rollout_bb_seq;
BlackBoxVectorEnv.rollout_sequence): up to S successive black-box steps (plan segments) of C parameter
sequences per env in one launch, from each env's current state, with the handle left untouched.

The yardstick is the existing step path: a twin env built with autoreset=False, loaded with the env's
state_dict() per candidate and stepped segment by segment; a pair's rows are recorded until its first
terminated | truncated segment, the rows after it are the padding (+0.0 / 0), `returns` is the host's
left-to-right f64 sum of the twin's segment returns.  Everything is compared bit for bit (NaNs
canonicalised, test_gpu_wide._bits).  Shapes: N = 200 (one partial workgroup per candidate) and
N = 300 (a full and a partial one, the last wave partial) with C in {1, 3}.  One section compares with
the CPU oracle instead, independently of the device's own step path."""
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
NS = "fgxrsq"
_REG = (registry.ENV_SPECS, registry._BB_IDS, registry.ALL_MOVEMENT_PRIMITIVE_ENVIRONMENTS,
        registry.MOVEMENT_PRIMITIVE_ENVIRONMENTS_FOR_NS)
FIELDS = ("returns", "lengths", "segments", "terminated", "truncated", "observations", "segment_returns",
          "segment_lengths")
SHAPES = [(200, 3), (300, 1), (300, 3)]


@pytest.fixture(scope="module", autouse=True)
def long_id():
    """fgxrsq252/LongSimpleReacher-v0: the registered spec with max_episode_steps = 252 (the plan then
    lasts 252 samples: step rewards in the workspace on SimpleReacher); this module only."""
    saved = [copy.deepcopy(d) for d in _REG]
    base = registry.ENV_SPECS["fancy/LongSimpleReacher-v0"]
    fgx.register(f"{NS}252/LongSimpleReacher-v0", base.kind, base.kwargs, max_episode_steps=252, mp_config=base.mp_config)
    yield
    for d, s in zip(_REG, saved):
        d.clear()
        d.update(s)


def _bb(**kw):
    return {"black_box_kwargs": kw}


# name: (env id, mp_config_override, scale of the N(0, 1) parameters)
CONFIGS = {
    "config5": ("fancy_ProDMP/SimpleReacher-v0", _bb(replanning_schedule=fgx.ReplanEvery(25)), 1.0),
    "hole25": ("fancy_ProDMP/HoleReacher-v0", _bb(replanning_schedule=fgx.ReplanEvery(25)), 10.0),
    "normperiod": ("fancy_ProMP/HoleReacher-v0",
                   _bb(replanning_schedule=fgx.ReplanEvery(40) | fgx.ReplanNormPeriod(16, 18, 30.0)), 1.0),
    "cond": ("fancy_ProDMP/SimpleReacher-v0",
             _bb(replanning_schedule=fgx.ReplanEvery(25), max_planning_times=3, condition_on_desired=True), 1.0),
    "promp_long": ("fancy_ProMP/LongSimpleReacher-v0", None, 1.0),
    "m252": (f"{NS}252_ProMP/LongSimpleReacher-v0", None, 1.0),
}


def _make(name, N, autoreset, over=None):
    env_id, base = CONFIGS[name][:2]
    return fgx.make(env_id, num_envs=N, device=DEV, mp_config_override=over or base, info_level=0, autoreset=autoreset)


def _start(name, N, pre=0, auto=False, seed=21):
    """The env under test after `pre` black-box steps (auto-resetting or not) and its twin (autoreset off)."""
    env = _make(name, N, auto)
    twin = _make(name, N, False)
    env.reset(seed=seed)
    g = torch.Generator().manual_seed(seed)
    for _ in range(pre):
        env.step((torch.randn(N, env.n_params, generator=g) * CONFIGS[name][2]).to(DEV))
    return env, twin


def _params(name, env, S, C, seed=5):
    p = np.random.default_rng(seed).standard_normal((S, C, env.num_envs, env.n_params)) * CONFIGS[name][2]
    return p.astype(np.float32)


def _step_path(env, twin, params, mean=False):
    """What the sequence rollout must give: per candidate the twin loaded with env's state and stepped
    segment by segment; rows recorded until the pair's first terminated | truncated."""
    S, C, N = params.shape[:3]
    sd = env.state_dict()
    w = dict(returns=np.zeros((C, N)), lengths=np.zeros((C, N), np.int32), segments=np.zeros((C, N), np.int32),
             terminated=np.zeros((C, N), bool), truncated=np.zeros((C, N), bool),
             observations=np.zeros((C, N, env.out_dim), np.float32), segment_returns=np.zeros((S, C, N)),
             segment_lengths=np.zeros((S, C, N), np.int32))
    for c in range(C):
        twin.load_state_dict(sd)
        run = np.ones(N, bool)
        for s in range(S):
            if not run.any():
                break
            obs, ret, te, tr, info = twin.step(torch.from_numpy(params[s, c]).to(DEV))
            obs, ret, te, tr, ln = np_(obs), np_(ret), np_(te), np_(tr), np_(info["trajectory_length"])
            w["segment_returns"][s, c, run] = ret[run]
            w["segment_lengths"][s, c, run] = ln[run]
            # the host's left-to-right f64 sum, starting from r_0
            w["returns"][c, run] = ret[run] if s == 0 else w["returns"][c, run] + ret[run]
            w["lengths"][c, run] += ln[run]
            w["segments"][c, run] = s + 1
            w["terminated"][c, run] = te[run]
            w["truncated"][c, run] = tr[run]
            w["observations"][c, run] = obs[run]
            run = run & ~(te | tr)
    return w


def _same(got, want, what="", only=None):
    got = got._asdict()
    for k, w in want.items():
        if got[k] is None:
            continue
        g = np_(got[k])
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what}{k}: {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        if only is not None:   # a [C, N] mask of the pairs to compare
            g, w = (g[:, only], w[:, only]) if k.startswith("segment_") else (g[only], w[only])
        diff = _bits(g) != _bits(w)
        assert not diff.any(), (f"{what}{k} differs in {int(diff.sum())} of {diff.size} bytes, first at "
                                f"{np.argwhere(diff)[0].tolist()} of {list(diff.shape)}")


def _run(env, p, **kw):
    return env.rollout_sequence(torch.from_numpy(p).to(DEV), **kw)


def _hist(M, S):
    return [np.bincount(m, minlength=S + 1)[1:].tolist() for m in M]


# ------------------------------------------------------------------------------------ 1. config 5
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-C%d" % s)
def test_config5_from_a_fresh_reset(shape):
    """8 segments of 25 samples make the episode: every pair runs M = 8 and is truncated; the ninth row
    is padding, and its parameters are never read."""
    N, C = shape
    env, twin = _start("config5", N)
    p = _params("config5", env, 9, C)
    want = _step_path(env, twin, p)
    assert (want["segments"] == 8).all() and want["truncated"].all() and not want["terminated"].any()
    assert (want["segment_lengths"][:8] == 25).all() and (want["lengths"] == 200).all()
    got = _run(env, p)
    assert got.terminated.dtype == torch.bool and got.truncated.dtype == torch.bool
    _same(got, want)
    assert (_bits(np_(got.segment_returns[8])) == _bits(np.zeros((C, N)))).all()   # +0.0, not -0.0
    assert (np_(got.segment_lengths[8]) == 0).all()
    p[8] = np.nan
    _same(_run(env, p), want, "NaN padding row: ")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-C%d" % s)
def test_config5_mid_episode(shape):
    N, C = shape
    env, twin = _start("config5", N, pre=3)
    assert (np_(env.get_state()["steps"]) == 75).all()
    p = _params("config5", env, 9, C)
    want = _step_path(env, twin, p)
    assert (want["segments"] == 5).all() and want["truncated"].all()
    _same(_run(env, p), want)
    # S = 3: nothing ends, the observation is the mid-episode one
    want3 = _step_path(env, twin, p[:3])
    assert (want3["segments"] == 3).all() and not (want3["truncated"] | want3["terminated"]).any()
    assert (want3["lengths"] == 75).all()
    got3 = _run(env, p[:3])
    _same(got3, want3)
    assert not np.array_equal(np_(got3.observations), want["observations"])


# ------------------------------------------------------------------------------------ 2. ragged ends
def _ragged(N, C):
    env, twin = _start("hole25", N)
    p = _params("hole25", env, 9, C)   # default_rng(5).standard_normal((9, C, N, n_params)) * 10
    return env, twin, p


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-C%d" % s)
def test_ragged_ends(shape):
    """Collisions end the pairs of a wave at different segments: finished lanes leave the segment loop
    while their neighbours run on."""
    N, C = shape
    env, twin, p = _ragged(N, C)
    want = _step_path(env, twin, p)
    M = want["segments"]
    print(f"hole25 {shape}: M histograms {_hist(M, 9)}, terminated {want['terminated'].sum(axis=1).tolist()}")
    for c in range(C):   # the batch is not degenerate
        assert len(set(M[c].tolist())) >= 4 and (M[c] < 9).all()
        assert want["terminated"][c].any() and want["truncated"][c].any()
    _same(_run(env, p), want)
    # the optional outputs left out (NULL pointers) while lanes leave the loop at different segments
    _same(_run(env, p, observations=False, segment_returns=False), want, "lean: ")


# ------------------------------------------------------------------------------------ 3. state-dependent schedule
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-C%d" % s)
def test_state_dependent_schedule(shape):
    N, C = shape
    env, twin = _start("normperiod", N, pre=2, auto=True)
    assert len(set(np_(env.get_state()["steps"]).tolist())) > 1   # envs sit at different step counts
    p = _params("normperiod", env, 4, C)
    want = _step_path(env, twin, p)
    L0 = want["segment_lengths"][0, 0, :64]
    assert len(set(L0.tolist())) > 1   # segment lengths differ inside a wave
    _same(_run(env, p), want)
    _same(_run(env, p, observations=False, segment_returns=False), want, "lean: ")


# ------------------------------------------------------------------------------------ 4. condition_on_desired
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-C%d" % s)
def test_condition_on_desired_carried_in_registers(shape):
    N, C = shape
    env, twin = _start("cond", N)
    p = _params("cond", env, 4, C)
    want = _step_path(env, twin, p)
    assert (want["segments"] == 3).all()
    assert (want["segment_lengths"][:3] == np.array([25, 25, 150], np.int32)[:, None, None]).all()
    _same(_run(env, p), want)
    env.step(torch.from_numpy(p[0, 0]).to(DEV))   # one step: a stored condition, plans = 1
    want = _step_path(env, twin, p)
    assert (want["segments"] == 2).all()
    _same(_run(env, p), want, "after one step: ")


# ------------------------------------------------------------------------------------ 5. ids without replanning
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-C%d" % s)
def test_without_replanning_it_is_rollout(shape):
    N, C = shape
    env, _ = _start("promp_long", N)
    p = _params("promp_long", env, 2, C)
    got = _run(env, p)
    one = env.rollout(torch.from_numpy(p[0]).to(DEV))
    assert (np_(got.segments) == 1).all()
    for a, b in zip((got.returns, got.lengths, got.terminated, got.truncated, got.observations), one):
        assert np.array_equal(_bits(np_(a)), _bits(np_(b)))
    assert np.array_equal(_bits(np_(got.segment_returns[0])), _bits(np_(one[0])))
    assert (np_(got.segment_lengths[1]) == 0).all()
    # and S = 1 on a replanning id
    env, _, p = _ragged(N, C)
    got = _run(env, p[:1])
    one = env.rollout(torch.from_numpy(p[0]).to(DEV))
    assert (np_(got.segments) == 1).all()
    for a, b in zip((got.returns, got.lengths, got.terminated, got.truncated, got.observations), one):
        assert np.array_equal(_bits(np_(a)), _bits(np_(b)))


# ------------------------------------------------------------------------------------ 6. long segments
def test_long_segments_through_the_workspace():
    N, C = 200, 3
    env, twin = _start("m252", N, seed=4)
    assert env.T == 252
    n = ctypes.c_int64()
    _lib.check(env._eng.lib.fgx_rollout_bb_workspace(env._eng.h, C, ctypes.byref(n)))
    assert n.value == 8 * C * 252 * N
    p = _params("m252", env, 2, C, seed=8)
    want = _step_path(env, twin, p)
    assert (want["segments"] == 1).all() and (want["lengths"] == 252).all()
    _same(_run(env, p), want)


# ------------------------------------------------------------------------------------ 7. non-finite parameters
@pytest.mark.parametrize("name", ["config5", "hole25"])
def test_non_finite_parameters_in_a_later_segment(name):
    N, C = 300, 3
    env, twin = _start(name, N)
    clean = _params(name, env, 9, C)
    p = clean.copy()
    p[1, 0, 7, 0] = np.nan          # a lane of a full wave
    p[1, 1, 70, 3] = np.inf
    p[1, 1, 299, 1] = -np.inf       # the partial last wave
    p[1, 2, 130, :] = np.nan        # a whole row
    hit = np.zeros((C, N), bool)
    hit[0, 7] = hit[1, 70] = hit[1, 299] = hit[2, 130] = True
    want = _step_path(env, twin, p)
    want_clean = _step_path(env, twin, clean)
    assert (want_clean["segments"][hit] >= 2).all()   # the hit pairs reach segment 1
    got = _run(env, p)
    _same(got, want)
    _same(got, want_clean, "other pairs: ", only=~hit)
    for k in ("segment_returns", "segment_lengths"):   # segment 0 of the hit pairs is the clean one
        assert np.array_equal(_bits(np_(getattr(got, k))[0][hit]), _bits(want_clean[k][0][hit])), k
    assert not np.isfinite(np_(got.returns)[hit]).all()


# ------------------------------------------------------------------------------------ 8. nothing changes
@pytest.mark.parametrize("name,pre,S", [("config5", 3, 9), ("hole25", 0, 9), ("cond", 1, 4)])
def test_sequence_rollout_leaves_the_handle_untouched(name, pre, S):
    N, C = 300, 3
    env, twin = _start(name, N, pre=pre)
    before = env.state_dict()["blob"].clone()
    _run(env, _params(name, env, S, C))
    after = env.state_dict()["blob"]
    assert torch.equal(before.view(torch.uint8), after.view(torch.uint8))
    # and the step that follows is the twin's step from the same state
    twin.load_state_dict(env.state_dict())
    twin.autoreset = env.autoreset
    p = torch.from_numpy(_params(name, env, 1, 1, seed=6)[0, 0]).to(DEV)
    a, b = env.step(p), twin.step(p)
    for x, y, k in zip(a[:4], b[:4], ("obs", "ret", "terminated", "truncated")):
        assert np.array_equal(_bits(np_(x)), _bits(np_(y))), k
    assert torch.equal(a[4]["trajectory_length"], b[4]["trajectory_length"])
    assert torch.equal(env.state_dict()["blob"].view(torch.uint8), twin.state_dict()["blob"].view(torch.uint8))


# ------------------------------------------------------------------------------------ 9. the CPU oracle
@pytest.mark.parametrize("name,pseed", [("config5", 31), ("hole25", 5)])
def test_sequence_rollout_vs_oracle(name, pseed):
    """BatchedBB stepped per candidate on a deep copy, each pair stopped at its first done (the oracle
    auto-resets after it).  Lengths, flags and M exact, segment returns within 16 ulp."""
    N, C, S = 128, 2, 8
    env_id, over, scale = CONFIGS[name]
    env = fgx.make(env_id, num_envs=N, device=DEV, mp_config_override=over, info_level=0)
    ob = batched.BatchedBB(env_id.split("/")[1][:-3], N, ctrl_of(env), mp_spec=spec_of(env), **oracle_kwargs(env))
    close(np_(env.reset(seed=9)[0]), ob.reset(seed=9))
    p = (np.random.default_rng(pseed).standard_normal((S, C, N, env.n_params)) * scale).astype(np.float32)
    got = _run(env, p)
    for c in range(C):
        o = copy.deepcopy(ob)
        run = np.ones(N, bool)
        M = np.zeros(N, np.int32)
        te_l, tr_l = np.zeros(N, bool), np.zeros(N, bool)
        obs_l = np.zeros((N, env.out_dim), np.float32)
        for s in range(S):
            if not run.any():
                break
            _, r_ret, r_te, r_tr, r_info = o.step(p[s, c])
            np.testing.assert_array_equal(np_(got.segment_lengths[s, c])[run], r_info["trajectory_length"][run])
            assert_ulps(np_(got.segment_returns[s, c])[run], r_ret[run], 16)
            M[run] = s + 1
            te_l[run], tr_l[run], obs_l[run] = r_te[run], r_tr[run], r_info["final_obs"][run]
            run = run & ~(r_te | r_tr)
            assert (np_(got.segment_lengths[s, c])[M < s + 1] == 0).all()
        np.testing.assert_array_equal(np_(got.segments[c]), M)
        np.testing.assert_array_equal(np_(got.terminated[c]), te_l)
        np.testing.assert_array_equal(np_(got.truncated[c]), tr_l)
        close(np_(got.observations[c]), obs_l)
        if name == "hole25":
            assert 0 < te_l.sum() < N and len(set(M.tolist())) >= 4


# ------------------------------------------------------------------------------------ 10. graph capture
def test_sequence_rollout_in_a_graph():
    N, C = 200, 3
    env, twin, p = _ragged(N, C)
    p = torch.from_numpy(p).to(DEV)
    env.rollout_sequence(p)   # (the workspace of this C is allocated outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = env.rollout_sequence(p)
    torch.cuda.current_stream().wait_stream(side)
    for i in range(2):
        env.step(p[i, 0])   # the state moves on
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        eager = env.rollout_sequence(p)
        for a, b in zip(out, eager):
            assert np.array_equal(_bits(np_(a)), _bits(np_(b))), f"replay {i}"


def test_first_sequence_rollout_inside_a_capture_is_refused():
    env, _ = _start("hole25", 64)
    p = torch.from_numpy(_params("hole25", env, 2, 2)).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with pytest.raises(RuntimeError, match="workspace"):
            with torch.cuda.graph(g, stream=side):
                env.rollout_sequence(p)
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------ 11. refusals and shapes
def _raw(env, p, S, C, ws=None, nbytes=0):
    N = env.num_envs
    shape = (max(C, 1), N)
    ret = torch.empty(shape, dtype=torch.float64, device=DEV)
    ln = torch.empty(shape, dtype=torch.int32, device=DEV)
    sg = torch.empty(shape, dtype=torch.int32, device=DEV)
    te = torch.empty(shape, dtype=torch.uint8, device=DEV)
    tr = torch.empty_like(te)
    v = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    return env._eng.lib.fgx_rollout_bb_seq(env._eng.h, v(p), S, C, v(ret), v(ln), v(sg), v(te), v(tr), None, None, None,
                                           v(ws) if ws is not None else None, nbytes, env._eng.stream())


def test_refusals_and_shapes():
    N = 64
    env = _make("hole25", N, False)
    P = env.n_params
    p = torch.zeros((3, 2, N, P), device=DEV)
    with pytest.raises(ResetNeeded):
        env.rollout_sequence(p)
    env.reset(seed=1)
    for bad in (torch.zeros((3, 2, N + 1, P)), torch.zeros((3, 2, N, P + 1)), torch.zeros((N, P)),
                torch.zeros((1, 3, 2, N, P)), torch.zeros((0, 2, N, P)), torch.zeros((3, 0, N, P))):
        with pytest.raises(ValueError, match="params"):
            env.rollout_sequence(bad)
    lib = env._eng.lib
    n = ctypes.c_int64()
    _lib.check(lib.fgx_rollout_bb_workspace(env._eng.h, 2, ctypes.byref(n)))
    assert n.value == 8 * 2 * env.T * N   # a direct env at T = 200 > 128
    ws = torch.empty(n.value // 8, dtype=torch.float64, device=DEV)
    assert _raw(env, p, 0, 2, ws, n.value) == -1 and b"n_seg" in lib.fgx_last_error()
    assert _raw(env, p, 3, 0, ws, n.value) == -1 and b"n_cand" in lib.fgx_last_error()
    assert _raw(env, p, 3, 2, ws, n.value - 8) == -1 and b"workspace" in lib.fgx_last_error()
    assert _raw(env, p, 3, 2, None, 0) == -1 and b"workspace" in lib.fgx_last_error()
    assert _raw(env, p, 3, 2, ws, n.value) == 0

    def refused(word, env_id, over=None, **kw):
        e = fgx.make(env_id, num_envs=8, device=DEV, mp_config_override=over, info_level=0, **kw)
        e.reset(seed=0)
        z = torch.zeros((2, 2, 8, e.n_params), device=DEV)
        with pytest.raises(ValueError, match=word):
            e.rollout_sequence(z)
        return e, z

    for word, over, kw in (("learn", {"phase_generator_kwargs": {"learn_tau": True}}, {}),
                           ("wide", {"basis_generator_kwargs": {"num_basis": 13}}, {}),
                           ("validity", None, dict(traj_validity=fgx.TrajValidity(pos_low=[-1.2] * 5, pos_high=[1.2] * 5)))):
        e, z = refused(word, "fancy_ProMP/LongSimpleReacher-v0", over, **kw)
        # (Python asks for the workspace first; the entry point itself refuses under its own name)
        assert _raw(e, z, 2, 2) == -4 and lib.fgx_last_error().startswith(b"fgx_rollout_bb_seq: ")
        assert word.encode() in lib.fgx_last_error()
    refused("reward_aggregation", "fancy_ProMP/LongSimpleReacher-v0", _bb(reward_aggregation=np.max))
    # a step-based handle has no movement primitive: the raw call on a StepVectorEnv's handle
    se = fgx.make("fancy/SimpleReacher-v0", num_envs=8, device=DEV)
    se.reset(seed=0)
    assert _raw(se, torch.zeros((1, 1, 8, 4), device=DEV), 1, 1) == -4   # FGX_E_UNSUPPORTED
    assert b"fgx_rollout_bb_seq" in lib.fgx_last_error() and b"movement primitive" in lib.fgx_last_error()


def test_one_candidate_form_options_and_mean():
    N = 200
    env, twin, p = _ragged(N, 1)
    four = _run(env, p)
    three = _run(env, p[:, 0])
    assert tuple(three.returns.shape) == (N,) and tuple(three.observations.shape) == (N, env.out_dim)
    assert tuple(three.segment_returns.shape) == (9, N) and tuple(three.segments.shape) == (N,)
    for a, b, k in zip(four, three, FIELDS):
        a = np_(a)
        assert np.array_equal(_bits(a[:, 0] if k.startswith("segment_") else a[0]), _bits(np_(b))), k
    lean = _run(env, p, observations=False, segment_returns=False)
    assert lean.observations is None and lean.segment_returns is None and lean.segment_lengths is None
    assert np.array_equal(_bits(np_(lean.returns)), _bits(np_(four.returns)))
    # np.mean: every segment's return is the step path's sum / length; returns their left-to-right sum
    over = dict(CONFIGS["hole25"][1])
    over["black_box_kwargs"] = dict(over["black_box_kwargs"], reward_aggregation=np.mean)
    em, tm = _make("hole25", N, False, over), _make("hole25", N, False, over)
    em.reset(seed=21)
    want = _step_path(em, tm, p)
    _same(_run(em, p), want)
    _same(_run(em, p, segment_returns=False), want)
