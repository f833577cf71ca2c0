"""The policy's host side (no GPU): irl_control_amd/policy.py -- the exact float32 fma the mirror is built on against libm's fmaf, the
mirror of the network against float64 and against a torch module's own forward, from_torch, the layout of the observation and the
struct of include/irlosc.h.

BOUNDS.  One layer with K inputs (padded: K' <= K + 3 steps, the padding adding exact zeros) is a chain of K' fused multiply-adds behind
the bias: every step rounds once, relative 2^-24, on a partial sum bounded by S = sum |w_i x_i| + |b|; so |mlp - exact| <= K' 2^-24 S (1 +
O(2^-24)), and (K + 2) 2^-24 S is asserted -- it holds because a step whose operands are zero rounds nothing, so at most K steps round, and
the float64 reference's own error, (K + 1) 2^-53 S, is eight orders below.  Against torch's CPU forward, which sums the same products in an
order of its own with the same unit roundoff per step, both sides are within that bound of the exact value: twice the bound, per layer;
for a deeper net the bound of a layer is taken on |W| |x| of the inputs it saw and propagated through the following layers' |W|."""
import ctypes as C
import ctypes.util
import itertools
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from irl_control_amd import _lib, policy, synth, teleop      # noqa: E402

F32 = np.float32
A_HEX, B_HEX, C_HEX = "0x1.00062ep-4", "0x1.3ec94ep-4", "0x1.0p+0"      # the triple on which the naive form double-rounds
U = 2.0 ** -24


def libm_fmaf():
    lib = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lib.fmaf.argtypes = [C.c_float] * 3
    lib.fmaf.restype = C.c_float
    return lib.fmaf


def fmaf_all(a, b, c):
    f = libm_fmaf()
    return np.array([f(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def triples(n, seed):
    """Random, cancelling and mixed-scale triples, n of each."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(F32)
    b = rng.standard_normal(n).astype(F32)
    c = rng.standard_normal(n).astype(F32)
    sets = [(a, b, c)]
    # cancelling: the addend is the product's negation up to a few ulp, so the result is the product's low part
    near = (-(a.astype(np.float64) * b)).astype(F32)
    sets.append((a, b, np.nextafter(near, F32(np.inf) * rng.choice([-1, 1], n).astype(F32)).astype(F32)))
    sets.append((a, b, near))
    # mixed scales: exponents spread over +-60 binades, the addend near the product's half-ulp boundary included
    sa, sb, sc = (np.ldexp(F32(1), rng.integers(-60, 60, n)).astype(F32) for _ in range(3))
    sets.append((a * sa, b * sb, c * sc))
    with np.errstate(over="ignore"):      # (an addend beyond float32's range is an infinity on both sides)
        sets.append((a * sa, b * sb, (a.astype(np.float64) * sa * b * sb * 2.0 ** rng.integers(20, 30, n)).astype(F32)))
    return sets


def test_fma32_equals_fmaf_on_random_cancelling_and_mixed_scale_triples():
    for a, b, c in triples(20000, 11):
        got, want = policy.fma32(a, b, c), fmaf_all(a, b, c)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, (a[bad[0]].hex(), b[bad[0]].hex(), c[bad[0]].hex(), got[bad[0]].hex(), want[bad[0]].hex())


def test_fma32_on_the_double_rounding_triple_where_the_naive_form_fails():
    a, b, c = (F32(float.fromhex(h)) for h in (A_HEX, B_HEX, C_HEX))
    want = libm_fmaf()(float(a), float(b), float(c))
    assert float(want).hex() == "0x1.013ed20000000p+0"
    assert float(policy.fma32(a, b, c)).hex() == float(want).hex()
    naive = F32(np.float64(a) * np.float64(b) + np.float64(c))
    assert float(naive).hex() == "0x1.013ed00000000p+0" and naive != F32(want)


def random_layers(dims, seed):
    rng = np.random.default_rng(seed)
    return [((rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32), rng.standard_normal(o).astype(F32)) for i, o in zip(dims[:-1], dims[1:])]


@pytest.mark.parametrize("K,O", [(1, 1), (6, 7), (31, 20), (128, 16), (192, 128)])
def test_mlp_single_layer_against_float64(K, O):
    (W, b), = random_layers([K, O], 100 + K)
    x = np.random.default_rng(K).standard_normal((9, K)).astype(F32)
    got = policy.mlp(x, [(W, b)]).astype(np.float64)
    W64, x64, b64 = W.astype(np.float64), x.astype(np.float64), b.astype(np.float64)
    exact = x64 @ W64.T + b64
    bound = (K + 2) * U * (np.abs(x64) @ np.abs(W64).T + np.abs(b64))
    assert got.shape == (9, O) and (np.abs(got - exact) <= bound).all(), np.max(np.abs(got - exact) / bound)


def test_mlp_order_shows_on_random_data():
    layers = random_layers([31, 20, 7], 5)
    x = np.random.default_rng(6).standard_normal((70, 31)).astype(F32)
    up, down = policy.mlp(x, layers), policy.mlp(x, layers, descending=True)
    assert (bits(up) != bits(down)).mean() >= 0.5


def test_from_torch_bit_for_bit_and_mlp_against_the_modules_forward():
    import torch
    torch.manual_seed(3)
    dims = [31, 20, 48, 7]
    mods = []
    for i, o in zip(dims[:-1], dims[1:]):
        mods += [torch.nn.Linear(i, o), torch.nn.ReLU()]
    net = torch.nn.Sequential(*mods[:-1])
    layers = policy.from_torch(net)
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    assert len(layers) == 3
    for (W, b), m in zip(layers, lin):
        assert W.dtype == F32 and b.dtype == F32
        assert np.array_equal(bits(W), bits(m.weight.detach().numpy())) and np.array_equal(bits(b), bits(m.bias.detach().numpy()))
    x = np.random.default_rng(8).standard_normal((33, 31)).astype(F32)
    with torch.no_grad():
        want = net(torch.from_numpy(x)).numpy().astype(np.float64)
    got = policy.mlp(x, layers).astype(np.float64)
    # twice the single-layer bound, layer by layer: a layer's error passes the following layers scaled by at most their |W| (ReLU is 1-Lipschitz)
    h = x.astype(np.float64)
    err = np.zeros_like(h)
    for W, b in layers:
        W64 = W.astype(np.float64)
        err = err @ np.abs(W64).T + 2 * (W.shape[1] + 2) * U * (np.abs(h) @ np.abs(W64).T + np.abs(b.astype(np.float64)))
        h = np.maximum(h @ W64.T + b, 0.0)
    assert (np.abs(got - want) <= err).all(), np.max(np.abs(got - want) / err)
    with pytest.raises(ValueError):
        policy.from_torch(torch.nn.Sequential(torch.nn.Linear(3, 3), torch.nn.Tanh(), torch.nn.Linear(3, 6)))


@pytest.mark.parametrize("cfg,nobj", [("k13", 2), ("k6", 0), ("r6", 1)])
def test_observe_layout_for_every_subset(cfg, nobj):
    lay = synth.make_layout(cfg)
    n, ndev, B = lay.n, lay.ndev, 3
    rng = np.random.default_rng(2)
    ch = dict(qpos=rng.standard_normal((B, n)), qvel=rng.standard_normal((B, n)), ee_pose=rng.standard_normal((B, ndev, 7)),
              targets=rng.standard_normal((B, ndev, 7)), wrench=rng.standard_normal((B, ndev, 6)), object_pose=rng.standard_normal((B, nobj, 8)))
    plate = rng.standard_normal((B, 6))
    flat = dict(ch, plate=plate, object_pose=ch["object_pose"][..., :7])
    names = [nm for nm in policy.OBS_BITS if nobj or nm != "object_pose"]
    for r in range(1, len(names) + 1):
        for sub in itertools.combinations(names, r):
            mask = policy.obs_mask(sub)
            got = policy.observe(mask, ch, plate)
            want = np.concatenate([flat[nm].reshape(B, -1) for nm in policy.OBS_BITS if nm in sub], axis=1).astype(F32)
            assert got.dtype == F32 and got.shape == (B, policy.obs_width(mask, n, ndev, nobj)) and np.array_equal(bits(got), bits(want)), sub
    assert policy.obs_mask(("plate", "qpos")) == _lib.OBS_PLATE | _lib.OBS_QPOS == policy.obs_mask(33)
    assert [policy.OBS[nm] for nm in policy.OBS_BITS] == [_lib.OBS_QPOS, _lib.OBS_QVEL, _lib.OBS_EE_POSE, _lib.OBS_TARGETS, _lib.OBS_WRENCH,
                                                         _lib.OBS_PLATE, _lib.OBS_OBJECT_POSE]


def test_struct_matches_the_header():
    # uint32 obs, int32 n_layers, width[4], n_out, keep_obs, grip_dev, nb_origin | float clip, int32 reserved | 3 doubles | the stream's rig
    assert C.sizeof(_lib.Policy) == 4 * 10 + 8 + 24 + 16 + 96 + 128 + 32
    assert (_lib.Policy.clip.offset, _lib.Policy.grip_close.offset, _lib.Policy.increment.offset, _lib.Policy.kind.offset) == (40, 48, 64, 72)
    for f in ("kind", "off_xyz", "off_quat", "heading_offset"):
        assert getattr(_lib.Policy, f).size == getattr(_lib.TeleopStream, f).size
    hdr = open(os.path.join(ROOT, "include", "irlosc.h")).read()
    for name, val in (("IRLOSC_POLICY_MAX_IN", _lib.POLICY_MAX_IN), ("IRLOSC_POLICY_MAX_WIDTH", _lib.POLICY_MAX_WIDTH),
                      ("IRLOSC_POLICY_MAX_LAYERS", _lib.POLICY_MAX_LAYERS), ("IRLOSC_ABI_VERSION", 3)):
        assert f"#define {name} " in hdr and int(hdr.split(f"#define {name} ")[1].split()[0]) == val
    layers = random_layers([6, 64, 64, 7], 1)
    rig = teleop.space_mouse_rig(synth.make_layout("k13"))
    d = policy.to_struct(layers, ("plate",), rig, nb_origin=5, clip=0.5, keep_obs=True, grip_dev=1, grip_close=-0.4, grip_open=0.4)
    assert (d.obs, d.n_layers, list(d.width), d.n_out, d.keep_obs, d.grip_dev, d.nb_origin) == (_lib.OBS_PLATE, 3, [64, 64, 0, 0], 7, 1, 1, 5)
    assert d.clip == 0.5 and (d.grip_close, d.grip_open, d.increment) == (-0.4, 0.4, teleop.INCREMENT)
    assert list(d.kind)[:3] == [f["kind"] for f in rig]
    w = policy.weights(layers)
    assert w.dtype == F32 and w.size == 6 * 64 + 64 + 64 * 64 + 64 + 64 * 7 + 7 and np.array_equal(w[:384].reshape(64, 6), layers[0][0])


def test_policy_tick_is_a_stream_step_on_the_clamped_output():
    layers = random_layers([6, 16, 7], 9)
    rig = teleop.space_mouse_rig(synth.make_layout("k13"))
    pose = np.array(teleop.ORIGIN)
    obs = pose.astype(F32)
    new, tgt, out, g = policy.policy_tick(pose, obs, layers, rig, clip=0.25, grip=(-0.4, 0.4))
    assert np.array_equal(bits(out), bits(policy.mlp(obs[None], layers)[0]))
    r = policy.clamp(out, 0.25)
    assert r.dtype == np.float64 and np.abs(r).max() <= 0.25 and np.array_equal(r, np.clip(out[:6], F32(-0.25), F32(0.25)).astype(np.float64))
    want_pose, want_tgt = teleop.stream_step(pose, r, rig)
    assert np.array_equal(new, want_pose) and np.array_equal(np.nan_to_num(tgt, nan=7.0), np.nan_to_num(want_tgt, nan=7.0))
    assert g == (-0.4 if out[6] > 0 else 0.4)
    assert np.array_equal(policy.clamp(out, 0.0), out[:6].astype(np.float64))
