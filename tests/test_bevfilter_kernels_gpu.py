"""jp_bev_track_filter (csrc/bevfilter.hip) against the plain-Python reference of tests/bevfilter_ref.py.  Every comparison is BYTE
equality of the rolled state (slots_i, slots_d, head) and the outputs (obj_slot, fstats) after every call of a chain: the integers
are exact, and the float64 values are single-rounded operations in the order the header states.  Before every call obj_slot and fstats
are filled with 0x7f bytes -- what comes back equal to the reference was written by the call -- and every call is made twice from the
same state and the two results compared byte for byte.

The kernel reads only tracks / kin / stats, so most cases synthesise those arrays: objects on a 5 m grid that drift by multiples of a
quarter metre and are measured with a jitter of a quarter metre (equal d^2 between pairs is common: the tie-break is exercised),
seen with some probability per frame (misses, coasting, ends, births), now and then under a new tracker id (the id switch), in a
random object order per frame.  Shapes (max_tracks, max_objects): (4, 4), the hand cases of tests/test_bevfilter_abi_cpu.py;
(8, 16), more objects than slots; (100, 70), more than one wave of objects and of candidate slots, ragged against 64; (256, 256),
the bound, every slot and object in use and more than 100 re-acquire candidates in one call; two cameras with different histories;
stats[0] negative and above max_objects; max_coast 0; gate 0; non-finite measurements.  One chain runs the real BevObjects ->
BevTracker -> BevTrackFilter on 64 x 64 maps."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from jperceiver_amd import ops                                                     # noqa: E402
from jperceiver_amd.apis import BevObjects, BevTracker, BevTrackFilter             # noqa: E402
from tests import bevfilter_ref as R                                               # noqa: E402

DEV = "cuda"
STATE = ("slots_i", "slots_d", "head")
OUT = STATE + ("obj_slot", "fstats")
PAR = dict(max_coast=3, min_hits=3, gate=2.0, meas_sigma=0.625, vel_sigma0=3.0, accel_sigma=0.5)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _call(tracks, kin, stats, state, M, S, par):
    """one jp_bev_track_filter call on a copy of `state` and poisoned outputs -> dict of numpy arrays (OUT)"""
    B = tracks.shape[0]
    st = {k: _dev(v) for k, v in state.items()}
    obj_slot = torch.full((B, M * 4), 0x7f, device=DEV, dtype=torch.uint8).view(torch.int32)
    fstats = torch.full((B, 8 * 4), 0x7f, device=DEV, dtype=torch.uint8).view(torch.int32)
    ops.call("jp_bev_track_filter", _dev(tracks), _dev(kin), _dev(stats), st["slots_i"], st["slots_d"], st["head"], obj_slot, fstats, B, M, S,
             par["max_coast"], par["min_hits"], par["gate"], par["meas_sigma"], par["vel_sigma0"], par["accel_sigma"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in {**st, "obj_slot": obj_slot, "fstats": fstats}.items()}


def _same(got, want, what):
    for name in OUT:
        x, w = got[name], want[name]
        assert x.dtype == w.dtype and x.shape == w.shape, (what, name, x.dtype, w.dtype, x.shape, w.shape)
        if x.tobytes() != w.tobytes():
            bad = np.argwhere(~((x == w) | ((x != x) & (w != w)))) if x.dtype == np.float64 else np.argwhere(x != w)
            at = tuple(bad[0]) if len(bad) else None
            raise AssertionError(f"{what}: {name} differs at {len(bad)} places (0: only in the sign of a zero or the bits of a NaN), first {at}: "
                                 f"got {x[at] if at else None}, want {w[at] if at else None}")


def _chain(frames, M, S, par, what):
    """frames: [(tracks, kin, stats)]; the GPU and the reference chained side by side, the GPU's own state goes on -> fstats per call"""
    state = R.zero_state(frames[0][0].shape[0], S)
    seen = []
    for k, (tr, kin, st) in enumerate(frames):
        oslot, fs, new = R.step(tr, kin, st, state, M, S, **par)
        a = _call(tr, kin, st, state, M, S, par)
        b = _call(tr, kin, st, state, M, S, par)
        for name in OUT:
            assert a[name].tobytes() == b[name].tobytes(), (what, k, name, "two runs differ")
        _same(a, {**new, "obj_slot": oslot, "fstats": fs}, (what, k))
        state = {n: a[n] for n in STATE}
        seen.append(fs)
    return seen


@functools.lru_cache(maxsize=None)
def _synth(seed, n_obj, n_frames, p_vis=0.85, p_switch=0.1, switch_all=(), bad=0.0, quant=0.25):
    """-> per frame the objects [(track_id, X, Z)] of one camera, as a tracker would number them (see the module docstring)"""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(n_obj)))
    pos = np.array([[5.0 * (k % side), 5.0 * (k // side)] for k in range(n_obj)])
    vel = rng.integers(-2, 3, (n_obj, 2)) * quant
    tid, next_tid, frames = [-1] * n_obj, 0, []
    for f in range(n_frames):
        rows = []
        for k in rng.permutation(n_obj).tolist():
            pos[k] += vel[k]
            if not rng.random() < p_vis:
                tid[k] = -1
                continue
            if tid[k] < 0 or f in switch_all or rng.random() < p_switch:
                tid[k], next_tid = next_tid, next_tid + 1
            X, Z = (pos[k] + rng.integers(-1, 2, 2) * quant).tolist()
            if rng.random() < bad:
                X, Z = ((float("nan"), Z), (X, float("inf")), (-float("inf"), float("nan")))[int(rng.integers(0, 3))]
            rows.append((tid[k], X, Z))
        frames.append(tuple(rows))
    return tuple(frames)


def _stack(cams, M):
    """cams: per camera the frames of _synth -> [(tracks, kin, stats)] per frame"""
    return [R.frame([list(c[k]) for c in cams], M) for k in range(len(cams[0]))]


def test_hand_cases_through_the_kernel():
    # the frames of tests/test_bevfilter_abi_cpu.py; sigmas 1 and 2 (r = 1, c0 = 4), no process noise, gate 5, max_coast 2
    par = dict(max_coast=2, min_hits=3, gate=5.0, meas_sigma=1.0, vel_sigma0=2.0, accel_sigma=0.0)
    hits = [[(7, 10.0, -3.0)]] * 3
    two = [[(1, -2.0, 0.0), (2, 2.0, 0.0)]] * 3
    cases = {
        "life cycle and coasting to the end": [[(7, 10.0, -3.0)], [(7, 14.0, -3.0)], [(7, 17.0, -3.0)], [(7, 20.0, -3.0)], [], [], [], []],
        "tentative miss": [[(7, 10.0, -3.0)], [(7, 14.0, -3.0)], [], [(8, 14.0, -3.0)]],
        "re-acquire after coasting": hits + [[], [], [(9, 11.0, -3.0)], [(9, 12.0, -3.0)]],
        "id switch, then far away": hits + [[(9, 11.0, -3.0)], [(9, 12.0, -3.0)], [(10, 30.0, -3.0)]],
        "on the gate": hits + [[(9, 13.0, 1.0)]],
        "tie between slots": two + [[(5, 0.0, 0.0)]],
        "tie between objects": [[(1, 0.0, 0.0)]] * 3 + [[(5, 2.0, 0.0), (6, -2.0, 0.0)]],
        "nearest pair first": [[(1, 0.0, 0.0), (2, 3.0, 0.0)]] * 3 + [[(5, 2.0, 0.0), (6, 5.0, 0.0)]],
        "non-finite": hits + [[(7, float("nan"), 0.0), (9, 10.5, -3.0)], [(9, float("inf"), -3.0)], [(9, 11.0, -3.0)]],
    }
    seen = {}
    for name, frames in cases.items():
        seen[name] = _chain([R.frame([f], 4) for f in frames], 4, 4, dict(par, gate=2.5) if name == "nearest pair first" else par, name)
    assert [f[0].tolist() for f in seen["life cycle and coasting to the end"]][2:] == [
        [1, 1, 0, 1, 0, 0, 0, 0], [1, 1, 0, 1, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 1, 0], [0] * 8]
    assert seen["re-acquire after coasting"][5][0].tolist() == [1, 1, 0, 0, 1, 0, 0, 0]
    assert seen["tie between slots"][3][0].tolist() == [2, 1, 1, 0, 1, 0, 0, 0] and seen["on the gate"][3][0].tolist() == [1, 1, 0, 0, 1, 0, 0, 0]
    # the tie itself, read back: slot 0 took the object, slot 1 coasts
    got, state = None, R.zero_state(1, 4)
    for f in two + [[(5, 0.0, 0.0)]]:
        got = _call(*R.frame([f], 4), state, 4, 4, par)
        state = {n: got[n] for n in STATE}
    assert got["slots_i"][0, :2, [0, 1, 2, 6]].T.tolist() == [[0, 2, 5, 0], [1, 3, 2, -1]] and got["obj_slot"][0].tolist() == [0, -1, -1, -1]
    # two slots, three objects, and a freed slot that waits for the next call
    ex = [[(1, 0.0, 0.0), (2, 10.0, 0.0), (3, 20.0, 0.0)], [(2, 10.0, 0.0), (3, 20.0, 0.0)], [(2, 10.0, 0.0), (3, 20.0, 0.0)]]
    fs = _chain([R.frame([f], 4) for f in ex], 4, 2, par, "exhaustion")
    assert [f[0].tolist() for f in fs] == [[2, 0, 0, 0, 0, 2, 0, 1], [1, 0, 0, 1, 0, 0, 1, 1], [2, 1, 0, 1, 0, 1, 0, 0]]


def test_more_objects_than_slots():
    frames = _stack([_synth(3, 14, 10, p_vis=0.8), _synth(4, 16, 10, p_vis=0.7, bad=0.05)], 16)
    fs = _chain(frames, 16, 8, PAR, "8 slots, 16 objects")
    assert all((f[:, 0] <= 8).all() for f in fs) and sum(int(f[:, 7].sum()) for f in fs) > 0 and sum(int(f[:, 6].sum()) for f in fs) > 0


def test_more_than_one_wave_ragged_against_64():
    # 70 objects, 100 slots; in frame 3 the tracker renumbers every object: more than 64 candidate slots and candidate objects
    frames = _stack([_synth(11, 70, 8, p_vis=0.97, p_switch=0.05, switch_all=(3,))], 70)
    fs = _chain(frames, 70, 100, PAR, "100 slots, 70 objects")
    assert frames[3][2][0, 0] > 64 and fs[3][0, 3] == 0 and fs[3][0, 4] > 64
    print("(100, 70):", [f[0].tolist() for f in fs])


def test_the_bound_256_slots_256_objects():
    # every object seen in every frame, from frame 2 on about half of them under a new id: 256 objects, more than 100 candidates
    frames = _stack([_synth(21, 256, 6, p_vis=1.0, p_switch=0.0, switch_all=(4,)), _synth(22, 256, 6, p_vis=0.9, p_switch=0.45)], 256)
    fs = _chain(frames, 256, 256, PAR, "256 slots, 256 objects")
    assert frames[4][2][0, 0] == 256 and fs[4][0, 0] == 256 and fs[4][0, 3] == 0 and fs[4][0, 4] >= 100
    assert (fs[0][:, 5] == frames[0][2][:, 0]).all() and all(f[1, 4] > 0 for f in fs[2:])
    print("(256, 256):", [f.tolist() for f in fs])


def test_two_cameras_with_different_histories():
    a = _synth(31, 20, 9, p_vis=0.8, bad=0.05)
    b = _synth(32, 45, 9, p_vis=0.6, p_switch=0.3)
    a = a[:4] + ((), ()) + a[6:]                                        # camera 0 sees nothing for two frames: everything coasts
    fs = _chain(_stack([a, b], 64), 64, 100, PAR, "two cameras")
    assert fs[4][0, 2] > 0 and fs[4][0, 5] == 0 and fs[4][1, 5] > 0 and any(f[0, 4] > 0 for f in fs[6:])


def test_a_count_out_of_range_is_clamped():
    # camera 0: stats[0] negative (nothing is read); camera 1: far above max_objects (all 16 rows are read, none beyond)
    cams = [_synth(41, 16, 6, p_vis=1.0, p_switch=0.0), _synth(42, 16, 6, p_vis=1.0, p_switch=0.0)]
    frames = _stack(cams, 16)
    for k, (tr, kin, st) in enumerate(frames):
        assert st[:, 0].tolist() == [16, 16]
        st[0, 0] = (-3, -(2 ** 31), 16, 0, -1, 16)[k]
        st[1, 0] = (16, 17, 2 ** 31 - 1, 66, 16, 1000)[k]
    fs = _chain(frames, 16, 32, PAR, "clamped count")
    assert [f[0, 0] for f in fs] == [0, 0, 16, 0, 0, 16] and all(f[1, 0] == 16 for f in fs)


@pytest.mark.parametrize("par", [dict(max_coast=0), dict(gate=0.0), dict(min_hits=1, max_coast=1, accel_sigma=0.0, vel_sigma0=0.0),
                                 dict(gate=7.5, max_coast=5, min_hits=2)], ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()))
def test_parameter_edges(par):
    frames = _stack([_synth(51, 40, 8, p_vis=0.75, p_switch=0.25), _synth(52, 64, 8, p_vis=0.9, p_switch=0.2, bad=0.03)], 64)
    fs = _chain(frames, 64, 70, {**PAR, **par}, par)
    if par.get("max_coast") == 0:
        assert all((f[:, 2] == 0).all() for f in fs) and sum(int(f[:, 6].sum()) for f in fs) > 0       # nothing ever coasts
    if par.get("gate") == 0.0:
        print("gate 0: re-acquired per call", [f[:, 4].tolist() for f in fs])
    if par.get("gate") == 7.5:
        assert sum(int(f[:, 4].sum()) for f in fs) > 0                  # a gate wider than the 5 m grid: neighbours compete


def _block(occ, *blocks):
    m = np.zeros((1, occ, occ), dtype=np.uint8)
    for r0, c0 in blocks:
        m[0, r0:r0 + 3, c0:c0 + 3] = 2
    return m


def test_real_chain_objects_tracker_filter():
    # 64 x 64 maps (cells of 0.625 m), identity poses, reach 1.  Blob A (rows 20..22, columns 10..12) stands still and is blanked in
    # frames 3 and 4; blob B (rows 40..42) moves one column a frame and in frame 5 jumps four cells (2.5 m: beyond reach, within the
    # gate of 3 m around its predicted place).  The tracker gives A a new id in frame 5 and B a new id in frame 5; the filter keeps both.
    occ, M, S = 64, 8, 16
    par = dict(max_coast=3, min_hits=3, gate=3.0, vel_sigma0=3.0, accel_sigma=0.5)
    bcol = [30, 31, 32, 33, 34, 38, 39, 40]
    maps = [_block(occ, *(([] if k in (3, 4) else [(20, 10)]) + [(40, bcol[k])])) for k in range(8)]
    bo, tr = BevObjects(1, occ, max_objects=M), BevTracker(1, occ, max_objects=M)
    flt = BevTrackFilter(1, max_objects=M, max_tracks=S, occ=occ, **par)
    assert flt.meas_sigma == 40.0 / occ and flt.tracks() == [[]] and flt.stats_host() == [dict(zip(R_FSTATS, [0] * 8))]
    eye = torch.eye(4, dtype=torch.float64, device=DEV).repeat(1, 1, 1)
    keep = ("tracks_i", "kin", "stats")

    def run():
        recs = []
        for m in maps:
            assert flt.update(tr.update(bo.find(_dev(m)), eye)) is flt
            rec = {n: getattr(tr, n).clone() for n in keep}
            rec.update({n: getattr(flt, n).clone() for n in ("slots_i", "slots_d", "obj_slot", "fstats")}, head=flt._head.clone(), labels=bo.labels.clone())
            recs.append(rec)
        torch.cuda.synchronize()
        return [{k: v.cpu().numpy() for k, v in r.items()} for r in recs]

    first = run()
    state = R.zero_state(1, S)
    fid_a, fid_b, trk_a, trk_b = [], [], [], []
    for k, r in enumerate(first):
        oslot, fs, state = R.step(r["tracks_i"], r["kin"], r["stats"], state, M, S, meas_sigma=40.0 / occ, **par)
        _same(r, {**state, "obj_slot": oslot, "fstats": fs}, ("real chain", k))
        oa, ob = int(r["labels"][0, 21, 11]), int(r["labels"][0, 41, bcol[k] + 1])
        fid_a.append(int(r["slots_i"][0, oslot[0, oa], 0]) if oa >= 0 else None)
        trk_a.append(int(r["tracks_i"][0, oa, 0]) if oa >= 0 else None)
        fid_b.append(int(r["slots_i"][0, oslot[0, ob], 0]))
        trk_b.append(int(r["tracks_i"][0, ob, 0]))
    print("tracker ids of A", trk_a, "of B", trk_b, "; filtered ids of A", fid_a, "of B", fid_b)
    assert trk_a[5] != trk_a[2] and trk_b[5] != trk_b[4] and trk_b[4] == trk_b[0]                # the tracker lost both
    assert [f for f in fid_a if f is not None] == [fid_a[0]] * 6 and fid_b == [fid_b[0]] * 8 and fid_a[0] != fid_b[0]
    assert first[3]["fstats"][0].tolist() == [2, 1, 1, 1, 0, 0, 0, 0] and first[5]["fstats"][0].tolist() == [2, 2, 0, 0, 2, 0, 0, 0]
    # the host read of the last frame
    rows = flt.tracks(dt=0.1)[0]
    plain = flt.tracks()[0]
    assert [r["track"] for r in rows] == sorted([fid_a[0], fid_b[0]]) and all(r["status"] == "confirmed" and r["misses"] == 0 for r in rows)
    for r, q in zip(rows, plain):
        assert list(r) == ["track", "status", "age", "hits", "misses", "id", "X_w", "Z_w", "vX_w", "vZ_w", "speed", "heading_deg", "X_sigma", "Z_sigma"]
        s = first[-1]["slots_i"][0, :, 0].tolist().index(r["track"])
        d = first[-1]["slots_d"][0, s]
        assert [r["X_w"], r["Z_w"], q["vX_w"], q["vZ_w"]] == d[:4].tolist() and r["vX_w"] == d[2] / 0.1 and r["id"] == first[-1]["slots_i"][0, s, 6]
        assert q["speed"] == math.hypot(d[2], d[3]) and r["heading_deg"] == math.degrees(math.atan2(d[2] / 0.1, d[3] / 0.1))
        assert r["X_sigma"] == math.sqrt(d[4]) and r["Z_sigma"] == math.sqrt(d[7]) and (r["age"], r["hits"]) == (8, 8 if r["track"] == fid_b[0] else 6)
    b_row = rows[[r["track"] for r in rows].index(fid_b[0])]
    assert b_row["vX_w"] > 0.0 and abs(b_row["vZ_w"]) < 1e-9           # B moves along +X only
    assert flt.stats_host()[0] == dict(zip(R_FSTATS, first[-1]["fstats"][0].tolist()))
    with pytest.raises(ValueError, match="tracker has"):
        flt.update(BevTracker(1, occ, max_objects=M + 1))
    # reset: no history, and the same frames give the same bytes again
    for x in (bo, tr, flt):
        x.reset()
    assert int(flt.slots_i.abs().sum()) == 0 and float(flt.slots_d.abs().sum()) == 0.0 and int(flt._head.abs().sum()) == 0 and flt.tracks() == [[]]
    again = run()
    for k in range(len(maps)):
        for n in first[k]:
            assert first[k][n].tobytes() == again[k][n].tobytes(), (k, n)


R_FSTATS = ("live", "confirmed", "coasting", "continued", "reacquired", "born", "ended", "dropped")
