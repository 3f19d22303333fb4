"""Complete engine snapshots (csrc/fgx_snapshot.h; state_dict / load_state_dict / copy_envs of both
vector envs): a restored env continues bit for bit, auto-reset draws included; envs copied within
or across handles continue like their sources (common random numbers); mismatched snapshots and
broken copy contracts are refused with the env untouched; a restore + step pair replays from a HIP
graph.  67 envs unless a case says otherwise: one full wave plus three lanes, no multiple of any
workgroup size.  Every comparison is torch.equal on the tensors' bytes (NaN-safe, -0 != +0)."""
import io

import pytest
import torch

import fancy_gym_crowd_amd as fgx
from fancy_gym_crowd_amd.vector_env import BlackBoxVectorEnv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 67
REPLAN3 = {"black_box_kwargs": {"replanning_schedule": fgx.ReplanEvery(25), "max_planning_times": 3,
                                "condition_on_desired": True}}
# (env id, mp_config_override, make kwargs, envs, N(0, 1) scale of the parameters / actions)
CONFIGS = {
    "promp_simple_shard": ("fancy_ProMP/SimpleReacher-v0", None, {"info_level": 0}, N, 1.0),
    "promp_simple_v2": ("fancy_ProMP/SimpleReacher-v0", None, {"info_level": 2}, 256, 1.0),
    "prodmp_simple_replan3_cond": ("fancy_ProDMP/SimpleReacher-v0", REPLAN3, {"info_level": 0}, N, 1.0),
    "promp_hole_vel_acc": ("fancy_ProMP/HoleReacher-v0", None, {"info_level": 0, "rew_fct": "vel_acc"}, N, 1.0),
    "dmp_via": ("fancy_DMP/ViaPointReacher-v0", None, {"info_level": 0}, N, 0.3),
    # step-based, velocity actions applied unclipped: N(0, 1) rad per step (dt = 0.01), so that arms
    # leave their joint limits / reach the ground (termination -> auto-reset) within a few steps
    "step_hole": ("fancy/HoleReacher-v0", None, {}, N, 100.0),
}
HOLE = "promp_hole_vel_acc"


def _make(name, num_envs=None, **extra):
    env_id, over, kw, n, _ = CONFIGS[name]
    return fgx.make(env_id, num_envs=num_envs or n, device=DEV, mp_config_override=over, **{**kw, **extra})


def _width(env):
    return env.n_params if isinstance(env, BlackBoxVectorEnv) else env.dof


def _params(name, env, steps, seed=11):
    """`steps` parameter / action arrays [num_envs, width] f32 from a seeded torch.Generator."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(env.num_envs, _width(env), generator=g) * CONFIGS[name][4]).to(DEV) for _ in range(steps)]


def _step(env, p):
    """One step's tensors: obs, return / reward, terminated, truncated and every tensor of the info
    (trajectory_length, final_observation, the per-step arrays of the info level)."""
    obs, ret, te, tr, info = env.step(p)
    out = {"obs": obs, "ret": ret, "terminated": te, "truncated": tr}
    out.update({k: v for k, v in info.items() if isinstance(v, torch.Tensor) and not k.startswith("_")})
    assert "final_observation" in out
    if isinstance(env, BlackBoxVectorEnv):
        assert "trajectory_length" in out
    return out


def _bits(t):
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype != torch.bool else t.to(torch.uint8)


def _same(a, b, rows_a=None, rows_b=None, what=""):
    """Two steps' tensors (or the given rows of them) equal byte for byte."""
    assert a.keys() == b.keys()
    for k in a:
        x = a[k] if rows_a is None else a[k][rows_a]
        y = b[k] if rows_b is None else b[k][rows_b]
        assert x.shape == y.shape and torch.equal(_bits(x), _bits(y)), f"{what}{k} differs"


def _resume_case(name, through_cpu=False):
    A = _make(name)
    plist = _params(name, A, 6)
    A.reset(seed=7)
    for p in plist[:2]:
        A.step(p)
    sd = A.state_dict()
    assert sd["format"] == 1 and sd["num_envs"] == A.num_envs and sd["env_id"] == CONFIGS[name][0]
    assert sd["needs_reset"] is False and sd["blob"].dtype == torch.uint8 and sd["blob"].device == A.device
    if through_cpu:
        buf = io.BytesIO()
        torch.save({**sd, "blob": sd["blob"].cpu()}, buf)
        buf.seek(0)
        sd = torch.load(buf)
        assert sd["blob"].device.type == "cpu"
    want = [_step(A, p) for p in plist[2:]]
    # the random streams matter only if some env is auto-reset inside these steps
    done = torch.stack([(w["terminated"] | w["truncated"]).any() for w in want])
    assert bool(done.any()), "no env finished an episode in the 4 steps"
    B = _make(name)                      # fresh: never reset
    B.load_state_dict(sd)
    for i, p in enumerate(plist[2:]):
        _same(want[i], _step(B, p), what=f"resumed env, step {i}: ")
    A.load_state_dict(sd)                # rewind
    for i, p in enumerate(plist[2:]):
        _same(want[i], _step(A, p), what=f"rewound env, step {i}: ")
    return A, B, want


@pytest.mark.parametrize("name", list(CONFIGS))
def test_resume_bit_exact(name):
    A, _, want = _resume_case(name)
    if name == "promp_simple_shard":
        assert A.episode_kernel() == "k_episode_jl"
    if name == "promp_simple_v2":
        assert A.episode_kernel() == "k_episode_v2" and "step_observations" in want[0]
    if name == "prodmp_simple_replan3_cond":
        # two plans of 25 steps, then the third (max_planning_times) runs to the time limit: the 4 steps
        # cross an episode end, and plan lengths of both kinds occur
        tl = torch.stack([w["trajectory_length"] for w in want])
        assert bool((tl == 25).any()) and bool((tl > 25).any())
        assert bool(torch.stack([w["truncated"] for w in want]).any())


def test_nonrandom_reset_after_restore():
    """The last start angle is part of the snapshot: reset(options={'random_start': False}) restores it."""
    A = _make(HOLE)
    plist = _params(HOLE, A, 2)
    A.reset(seed=7)
    for p in plist:
        A.step(p)
    sd = A.state_dict()
    A.step(plist[0])                     # moves on: other start angles
    B = _make(HOLE)
    B.load_state_dict(sd)
    A.load_state_dict(sd)
    oa, _ = A.reset(options={"random_start": False})
    ob, _ = B.reset(options={"random_start": False})
    assert torch.equal(_bits(oa), _bits(ob))
    fresh = _make(HOLE)                  # (an env without the snapshot starts elsewhere)
    of, _ = fresh.reset(options={"random_start": False})
    assert not torch.equal(_bits(of), _bits(ob))


def test_copy_envs_fanout():
    """Envs 0..3 copied to 31 destinations each: every copy continues like its source, through an
    auto-reset (the copied stream draws the same hole and goal); the sources continue like a twin."""
    n = 128
    E, T = _make(HOLE, n), _make(HOLE, n)
    p0, p1, p2 = _params(HOLE, E, 3)
    dst = torch.arange(4, n, device=DEV)
    src = (dst - 4) // 31
    assert torch.bincount(src).tolist() == [31] * 4
    for env in (E, T):
        env.reset(seed=7)
        env.step(p0)
    E.copy_envs(src, dst)
    for i, p in enumerate((p1, p2)):
        p = p.clone()
        p[dst] = p[src]
        e, t = _step(E, p), _step(T, p)
        assert bool((e["terminated"] | e["truncated"])[:4].all())   # each step ends with an auto-reset
        _same(e, e, dst, src, what=f"step {i}, copies vs sources: ")
        _same(e, t, slice(0, 4), slice(0, 4), what=f"step {i}, sources vs twin: ")
        assert not torch.equal(_bits(e["obs"][4:]), _bits(t["obs"][4:]))   # the copy changed the destinations


def test_copy_envs_across_handles():
    S, D, T = _make(HOLE, 67), _make(HOLE, 130), _make(HOLE, 130)
    ps, pd = _params(HOLE, S, 3, seed=5), _params(HOLE, D, 3, seed=6)
    S.reset(seed=1000)
    S.step(ps[0])
    for env in (D, T):
        env.reset(seed=7)
        env.step(pd[0])
    # a source of another configuration is refused, the destination untouched (it still equals the twin below)
    other = _make(HOLE, 67, n_links=4)
    other.reset(seed=3)
    with pytest.raises(ValueError):
        D.copy_envs([5, 66], [129, 0], source=other)
    src, dst = [5, 66], [129, 0]
    D.copy_envs(src, dst, source=S)
    rest = slice(1, 129)
    for i in (1, 2):
        p = pd[i].clone()
        p[dst] = ps[i][src]
        s, d, t = _step(S, ps[i]), _step(D, p), _step(T, pd[i])
        _same(d, s, dst, src, what=f"step {i}, copies vs sources: ")
        _same(d, t, rest, rest, what=f"step {i}, untouched rows vs twin: ")


def test_load_state_dict_mismatch():
    E, T = _make(HOLE), _make(HOLE)
    p0, p1, p2 = _params(HOLE, E, 3)
    for env in (E, T):
        env.reset(seed=7)
        env.step(p0)
    own = E.state_dict()
    more = _make(HOLE, N + 1)
    more.reset(seed=9)
    other = _make(HOLE, N, n_links=4)
    other.reset(seed=9)
    for bad in (more.state_dict(), other.state_dict(), {**own, "format": 2}):
        with pytest.raises(ValueError):
            E.load_state_dict(bad)
    for i, p in enumerate((p1, p2)):
        _same(_step(E, p), _step(T, p), what=f"step {i} after the refused loads: ")


def test_copy_envs_contract():
    E, T = _make(HOLE), _make(HOLE)
    p0, p1 = _params(HOLE, E, 2)
    for env in (E, T):
        env.reset(seed=7)
        env.step(p0)
    for src, dst in (([0, 1], [5, 5]),          # a destination twice
                     ([0, 1], [5, N]),          # destination out of range
                     ([N, 1], [5, 6]),          # source out of range
                     ([-1, 1], [5, 6]),
                     ([0, 1], [1, 5])):         # env 1 is source and destination
        with pytest.raises(ValueError):
            E.copy_envs(src, dst)
    with pytest.raises(ValueError):
        E.copy_envs([0, 1, 2], [5, 6])
    E.copy_envs([], [])                         # nothing to do
    _same(_step(E, p1), _step(T, p1), what="after the refused copies: ")


def test_state_dict_roundtrip_through_cpu():
    _resume_case("promp_simple_shard", through_cpu=True)


def test_restore_then_step_in_graph():
    """fgx_restore of a fixed blob followed by step_into, captured as one linear HIP graph: every
    replay rewinds and steps again, so two replays and an eager restore + step give the same bytes."""
    name = "promp_simple_shard"
    env = _make(name)
    p = _params(name, env, 3)
    env.reset(seed=7)
    env.step(p[0])
    env.step(p[1])
    sd = env.state_dict()
    n = env.num_envs
    obs = torch.empty((n, env.out_dim), dtype=torch.float32, device=DEV)
    out = {"obs": obs, "fobs": torch.empty_like(obs), "ret": torch.empty(n, dtype=torch.float64, device=DEV),
           "te": torch.empty(n, dtype=torch.uint8, device=DEV), "tr": torch.empty(n, dtype=torch.uint8, device=DEV),
           "tl": torch.empty(n, dtype=torch.int32, device=DEV)}

    def rewind_and_step():
        env.load_state_dict(sd)          # blob on the env's device: one launch, nothing else
        env.step_into(p[2], out["obs"], out["ret"], out["te"], out["tr"], out["tl"], out["fobs"])

    def snap():
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items()}

    rewind_and_step()
    eager = snap()
    assert bool((eager["te"] | eager["tr"]).any())
    env.step(p[0])                       # leave the snapshot's state behind
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rewind_and_step()
    for v in out.values():
        v.zero_()
    g.replay()
    first = snap()
    for v in out.values():
        v.zero_()
    g.replay()
    second = snap()
    _same(first, eager, what="first replay vs eager: ")
    _same(second, first, what="second replay vs first: ")
