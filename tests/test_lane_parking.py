"""The lane-form eigen pass parks the head of A's triangle in LDS at a group's first load and reloads only the tail from the record
(csrc/osc_lane.hpp).  The parked values are the doubles that used to be read again, so nothing may change -- and nothing parked may
survive from one step, slot, block or group of records to the next.  Held here at the shapes where the eigen pass's parking could go
wrong: a last wave with 37 live lanes, both tiers (k7: every entry of A fits), trains on both banks, the fused path's blocks, and a
block of the eigen pass that takes a second group of records into the LDS of its first."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import oracle_on_all
from irl_control_amd import _lib, synth
from oracle import osc_oracle
from test_gpu_parity import _from_q_setup, in_parity_domain, rel_err
from test_resident_lane import _physical, _train_equals_single_step, _upload
from test_resident_lane_edges import _check_oracle, _n_flagged

pytestmark = pytest.mark.gpu

TOL64 = 1e-5
LANE_MIN_B = 4096
B_RAGGED = LANE_MIN_B + 37          # 64 full waves and one with 37 live lanes
B_EIG = 32768


# ---- 1. the resident lane route with a partial last wave -------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", ["k13", "k12_admit", "k7"])
def test_resident_lane_route_with_a_partial_last_wave(cfg):
    """Physical records from the front end, B = 4 096 + 37, tiers (1, 6, 6) [k13; k12 + admittance with a wrench] and (1, 3, 3) [k7]:
    the lane route, the oracle on every robot (<= 1e-5 on the parity domain, the reference's branch), flags equal to the row16 route's
    (a context created with IRLOSC_RESIDENT_LANE=0)."""
    B = B_RAGGED
    lay, gains, _, osc, rec = _physical(cfg, B, seed=901)
    assert osc.slot_route(0) == "lane", osc.slot_route(0)
    u, fl = osc.step(return_flags=True)
    osc.close()
    _, _, _, r16, rec2 = _physical(cfg, B, seed=901, lane=False)
    assert np.array_equal(rec2["M"], rec["M"]) and np.array_equal(rec2["J"], rec["J"])
    assert r16.slot_route(0) == "row16_tree"
    _, fl_r = r16.step(return_flags=True)
    r16.close()
    err, dom = _check_oracle(lay, gains, rec, u, fl, cfg)
    print(f"{cfg}: B {B}, max rel vs oracle {err:.2e} on {int(dom.sum())} robots, eigen path {_n_flagged(fl)}")
    assert dom[B - 37:].any()                 # (the last wave is checked too)
    assert np.array_equal(fl, fl_r)


# ---- 2. trains equal single steps ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", ["k13", "k7"])
def test_trains_on_both_banks_equal_single_steps(cfg):
    """Two slots with different records, 16 resident steps = two trains, one per bank: the last outputs equal a single step on the same
    slot bit for bit, from either first slot -- what one step, slot or block parked is not seen by the next."""
    B = B_RAGGED
    _, _, _, osc, _ = _physical(cfg, B, seed=902, n_slots=2)
    _, _, _, o2, rec1 = _physical(cfg, B, seed=903)
    o2.close()
    _upload(osc, rec1, slot=1)
    assert [osc.slot_route(s) for s in range(2)] == ["lane", "lane"]
    u0 = osc.step(slot=0)
    u1 = osc.step(slot=1)
    assert not np.array_equal(u0, u1)
    for first in (0, 1):
        _train_equals_single_step(osc, 2, 16, first, B)
    osc.close()


# ---- 3. the fused path: the same kernel on the walk's blocks ---------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", ["k13", "k7"])
def test_fused_step_with_a_partial_last_wave(cfg):
    """step_q at B = 4 096 + 37 against the chained oracles: oracle/osc_oracle.py on the front end's dense records of the same states
    on every robot, and oracle/rigid_body.py -> oracle/osc_oracle.py on the first and the last eight robots (the last wave's)."""
    from irl_control_amd.rigid_body import DUAL_UR5_EE
    from oracle import rigid_body as rb
    B = B_RAGGED
    lay, gains, g, model, osc, states = _from_q_setup(cfg, B, np.float64, seed=904, singular_every=7)
    assert "osc_lane" in osc.from_q_name, osc.from_q_name
    u, fl = osc.step_q(return_flags=True)
    assert np.all(np.isfinite(u)) and not np.any(fl & (_lib.FLAG_NONFINITE | _lib.FLAG_M_NOT_PD))
    osc.frontend()
    rec = osc.download_records(0)
    osc.close()
    rec["tgt_pose"] = g["tgt_pose"]
    ref, dom, pinv, trunc, _ = oracle_on_all(lay.as_oracle_dict(), gains, rec)
    err = rel_err(u, ref)
    print(f"{cfg}: fused step, B {B}, max rel vs oracle {err[dom].max():.2e} on {int(dom.sum())} robots, eigen path {_n_flagged(fl)}")
    assert dom.mean() > 0.9 and dom[B - 37:].any()
    assert err[dom].max() <= TOL64, float(err[dom].max())
    assert np.array_equal((fl[dom] & _lib.FLAG_PINV_BRANCH) != 0, pinv[dom])
    assert np.array_equal((fl[dom] & _lib.FLAG_TRUNCATED) != 0, trunc[dom])
    qpos, qvel = states[0]
    idx = np.r_[0:8, B - 8:B]
    om = rb.Model()
    recs = [rb.records(om, lay.as_oracle_dict(), DUAL_UR5_EE, qpos[b], qvel[b]) for b in idx]
    R = {k: np.array([r[k] for r in recs]) for k in ("M", "J", "dq", "bias", "ee_pose")}
    ref_c = osc_oracle.generate_batch(lay.as_oracle_dict(), gains, R["M"], R["J"], R["dq"], R["bias"], R["ee_pose"], g["tgt_pose"][idx])
    dom_c = np.array([in_parity_domain(*osc_oracle.task_inertia(R["J"][i], R["M"][i])[2:]) for i in range(len(idx))])
    assert dom_c.sum() >= len(idx) // 2 and rel_err(u[idx], ref_c)[dom_c].max() <= TOL64


# ---- 4. the lane-form eigen pass (from 3 000 flagged robots by default: forced, in child processes) ------------------------------------

def _eig_child(B, seed, out, save_records):
    lay, gains, _, osc, rec = _physical("k13", B, seed=seed)
    assert osc.slot_route(0) == "lane", osc.slot_route(0)
    res = {}
    res["u"], res["f"] = osc.step(return_flags=True)
    osc.close()
    if save_records:
        res.update({"r_" + k: v for k, v in rec.items() if k not in ("qpos", "qvel")})
    np.savez(out, **res)


def _run_child(tmp_path, name, B, seed, env_extra, save_records):
    """One setting of the eigen pass in a fresh process (it reads its environment once per process), under its own time limit."""
    out = str(tmp_path / f"{name}.npz")
    env = dict(os.environ)
    for k in ("IRLOSC_LANE_EIG_MIN", "IRLOSC_LANE_EIG_BLOCKS"):
        env.pop(k, None)
    env.update(env_extra)
    args = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
        [os.path.abspath(__file__), "--eig-child", str(B), str(seed), out, "1" if save_records else "0"]
    p = subprocess.run(args, env=env, cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (name, p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return dict(np.load(out))


def test_lane_form_eigen_pass_on_a_short_list(tmp_path):
    """IRLOSC_LANE_EIG_MIN=0 at B = 4 096 + 37: the few hundred flagged robots go through the lane-form pass (a last group with idle
    lanes, which carry the last live lane's offset into LDS); the oracle on every robot."""
    run = _run_child(tmp_path, "short", B_RAGGED, 905, {"IRLOSC_LANE_EIG_MIN": "0"}, True)
    lay = synth.make_layout("k13")
    _, gains, _ = synth.make_batch("k13", 2, seed=1, dtype=np.float64)
    rec = {k[2:]: v for k, v in run.items() if k.startswith("r_")}
    n = _n_flagged(run["f"])
    assert 64 < n < 3000 and n % 64 != 0, n
    err, dom = _check_oracle(lay, gains, rec, run["u"], run["f"], "lane-form eigen pass, short list")
    flagged = (run["f"] & _lib.FLAG_EIGEN_PATH) != 0
    print(f"lane-form eigen pass on {n} flagged robots of {B_RAGGED}: max rel vs oracle {err:.2e} ({int((dom & flagged).sum())} of them in the domain)")
    assert (dom & flagged).sum() > n // 4


def test_a_block_of_the_eigen_pass_that_takes_a_second_group(tmp_path):
    """B = 32 768, IRLOSC_LANE_EIG_MIN=0: more than 64 x 64 flagged robots, so with IRLOSC_LANE_EIG_BLOCKS=64 some blocks park a second
    group's A over their first's; with 1 024 blocks no block takes two.  Bit for bit the same torques and flags: a robot's result does
    not depend on which block or wave-mates it had."""
    runs = {}
    for name, blocks in (("capped", "64"), ("wide", "1024")):        # one at a time; the test stops at the first that fails
        runs[name] = _run_child(tmp_path, name, B_EIG, 906, {"IRLOSC_LANE_EIG_MIN": "0", "IRLOSC_LANE_EIG_BLOCKS": blocks}, False)
    n = _n_flagged(runs["wide"]["f"])
    print(f"{n} flagged robots of {B_EIG}: {-(-n // 64)} groups on 64 blocks")
    assert n > 64 * 64, n
    assert np.all(np.isfinite(runs["wide"]["u"]))
    assert np.array_equal(runs["capped"]["f"], runs["wide"]["f"])
    assert np.array_equal(runs["capped"]["u"], runs["wide"]["u"])


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--eig-child":
        _eig_child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5] == "1")
    else:
        sys.exit("usage: test_lane_parking.py --eig-child B SEED OUT.npz SAVE_RECORDS")
