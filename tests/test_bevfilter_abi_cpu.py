"""CPU-side checks of the filtered BEV tracks (csrc/bevfilter.hip, apis/bevfilter.py BevTrackFilter,
PerceptionStream(objects=dict(track=dict(filter=...)))): the entry point is declared in the header, exported by the library and bound,
with the documented argument names and types; the ABI version is unchanged (the change is additive); the header states what a caller
has to know; every refusal returns -1 with a message that names the argument before anything touches a device; `BevTrackFilter` and
the session refuse what they cannot run; and the reference the GPU tests compare against (tests/bevfilter_ref.py) is itself checked
against cases worked out by hand in the comments.  The hand cases hand the reference VARIANCES that are exact binary numbers:
r = 1, c0 = 2, q = 0 and gate^2 = 25 (no sigma squares to 2; the squaring itself is one multiply and is checked on its own)."""
import ctypes
import inspect
import math
import re
import subprocess

import numpy as np
import pytest
import torch

from jperceiver_amd import _lib
from tests import bevfilter_ref as R

P = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: validation comes first
NAMES = ["tracks", "kin", "stats", "slots_i", "slots_d", "head", "obj_slot", "fstats", "B", "max_objects", "max_tracks", "max_coast",
         "min_hits", "gate", "meas_sigma", "vel_sigma0", "accel_sigma", "stream"]
TYPES = ["const int*", "const double*", "const int*", "int*", "double*", "int*", "int*", "int*", "int", "int", "int", "int", "int",
         "double", "double", "double", "double", "void*"]
POINTERS = [n for n, t in zip(NAMES, TYPES) if t.endswith("*") and n != "stream"]
F = np.float64


def test_symbol_is_declared_exported_and_bound():
    L = _lib.lib()
    protos = _lib.parse_header()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (jp_\w+)", out))
    assert "jp_bev_track_filter" in protos and "jp_bev_track_filter" in exported and "jp_bev_track_filter" in L.fn
    assert L.fn["jp_abi_version"]() == 3
    assert [a for _, a in protos["jp_bev_track_filter"][1]] == NAMES
    assert [t for t, _ in protos["jp_bev_track_filter"][1]] == TYPES
    assert protos["jp_bev_track_filter"][0] == "int"
    i32, f64 = torch.int32, torch.float64
    assert L.ptr_dtypes["jp_bev_track_filter"][:8] == [i32, f64, i32, i32, f64, i32, i32, i32]


def test_header_states_what_a_caller_has_to_know():
    text = " ".join(open(_lib.HEADER_PATH).read().split()).replace(" * ", " ")
    block = text[text.index("Filtered BEV tracks"):text.index("jp_bev_track_filter(const int* tracks")]
    for sentence in (
            "TIE-BREAK: the smaller slot index, then the smaller object id",
            "slots that were free at entry of the call",
            "ZEROED STATE MEANS NO HISTORY",
            "slots_i (B,S,8) int32, row s = [fid, status, src_track, age, hits, misses, obj, 0]",
            "status 0 free, 1 tentative, 2 confirmed, 3 coasting",
            "slots_d (B,S,10) float64, row s = [X, Z, vX, vZ, aX, bX, cX, aZ, bZ, cZ]",
            "head (B,2) int32 = [next_fid, calls]",
            "obj_slot (B,M) int32",
            "fstats (B,8) int32 = [live, confirmed, coasting, continued, reacquired, born, ended, dropped]",
            "n = min(max(stats[b][0], 0), M)",
            "it is VALID iff both are finite",
            "No value read from device memory is used as an index before it is range-checked; track ids are only compared",
            "a' = ((a + (b + b)) + c) + q/4, b' = (b + c) + q/2, c' = c + q",
            "s is live with misses == 0 and src_track == t_c",
            "from the PREDICTED position",
            "a pair qualifies iff d2 <= gate gate (false for NaN)",
            "a match rebinds src_track = t_c",
            "each takes fid = next_fid++ in that order",
            "counted in dropped and take no fid",
            "covariance [[r, 0], [0, c0]]",
            "y = z - p', S = a' + r, K1 = a' / S, K2 = b' / S, p = p' + K1 y, v = v' + K2 y, a = a' - K1 a', b = b' - K1 b', c = c' - K2 b'",
            "a tentative slot, or one with misses + 1 > max_coast, is freed",
            "misses++, age++, status = 3, obj = -1",
            "2 if hits >= min_hits, else 1",
            "each squared once inside the call, one rounded multiply",
            "every operation rounded once (no fma)",
            "two runs give the same bytes",
            "ONE launch with fixed arguments",
            "no atomics, no workspace; no workgroup waits on another",
            "ORDERING in a session: jp_bev_track_filter behind jp_bev_tracks",
            "resetting the tracker without resetting the filter lets stale src_track values match new tracks"):
        assert sentence in block, sentence


def _rejected(L, *args):
    L.fn["jp_set_last_error"](b"")
    rc = L.fn["jp_bev_track_filter"](*args)
    assert rc == -1, (args, rc)
    msg = L.last_error()
    assert msg, args
    return msg


def test_bev_track_filter_rejects_bad_arguments():
    L = _lib.lib()
    good = [P, P, P, P, P, P, P, P, 2, 64, 128, 3, 3, 2.0, 0.15625, 3.0, 0.5, None]
    idx = {n: i for i, n in enumerate(NAMES)}

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[idx[k]] = v
        return _rejected(L, *a)

    for name in POINTERS:
        msg = bad(**{name: None})
        assert "null" in msg and name in msg, name
    for name in ("B", "max_objects", "max_tracks"):
        for v in (0, -3):
            msg = bad(**{name: v})
            assert "positive" in msg and name in msg
    for v in (257, 4096):
        msg = bad(max_objects=v)
        assert "max_objects" in msg and "256" in msg
        msg = bad(max_tracks=v)
        assert "max_tracks" in msg and "256" in msg
    for v in (-1, -100):
        assert "max_coast" in bad(max_coast=v)
    for v in (0, -2):
        assert "min_hits" in bad(min_hits=v)
    for name in ("gate", "meas_sigma", "vel_sigma0", "accel_sigma"):
        for v in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-300):
            assert name in bad(**{name: v}), (name, v)
    assert "meas_sigma" in bad(meas_sigma=0.0) and "greater than zero" in bad(meas_sigma=0.0)
    msg = bad(B=1 << 23, max_tracks=256, max_objects=1)                # B S 10 = 10 * 2^31
    assert "max_tracks" in msg and "2^31" in msg
    msg = bad(B=1 << 21, max_objects=256, max_tracks=1)                # B M 4 = 2^31
    assert "max_objects" in msg and "2^31" in msg
    assert "positive" in bad(stream=None, B=0)                          # the stream may be null (the default stream)


def test_python_surface_refuses_what_it_cannot_run():
    from jperceiver_amd import apis
    from jperceiver_amd.apis import BevTrackFilter, PerceptionStream
    from jperceiver_amd.apis.bevfilter import _filter_kw
    from jperceiver_amd.apis.bevobj import _objects_kw
    from jperceiver_amd.apis.bevtrack import _track_kw
    from jperceiver_amd.model import MONO
    from oracle import jp_oracle as J
    assert "BevTrackFilter" in apis.__all__
    sig = inspect.signature(BevTrackFilter.__init__).parameters
    assert list(sig) == ["self", "cameras", "max_objects", "max_tracks", "max_coast", "min_hits", "gate", "meas_sigma", "vel_sigma0",
                         "accel_sigma", "occ", "device"]
    assert [sig[k].default for k in list(sig)[2:]] == [64, None, 3, 3, 2.0, None, 3.0, 0.5, None, "cuda"]
    for name in ("update", "tracks", "stats_host", "reset"):
        assert callable(getattr(BevTrackFilter, name)), name
    with pytest.raises(TypeError, match="no CPU path"):
        BevTrackFilter(1, occ=64, device="cpu")
    with pytest.raises(TypeError, match="no CPU path"):
        BevTrackFilter(1, meas_sigma=0.5, device="cpu")
    with pytest.raises(ValueError, match="meas_sigma or occ"):
        BevTrackFilter(1, device="cpu")
    for kw, what in ((dict(max_objects=0), "max_objects"), (dict(max_objects=257), "max_objects"), (dict(max_tracks=0), "max_tracks"),
                     (dict(max_tracks=257), "max_tracks"), (dict(max_coast=-1), "max_coast"), (dict(min_hits=0), "min_hits"),
                     (dict(gate=-1.0), "gate"), (dict(gate=float("nan")), "gate"), (dict(meas_sigma=0.0), "meas_sigma"),
                     (dict(meas_sigma=float("inf")), "meas_sigma"), (dict(vel_sigma0=-1.0), "vel_sigma0"),
                     (dict(accel_sigma=float("nan")), "accel_sigma")):
        with pytest.raises(ValueError, match=what):
            BevTrackFilter(1, occ=64, device="cpu", **kw)
    with pytest.raises(ValueError, match="positive"):
        BevTrackFilter(0, occ=64, device="cpu")
    # the argument checks of update and tracks fire before anything is enqueued
    f = BevTrackFilter.__new__(BevTrackFilter)
    f.cameras, f.max_objects = 2, 8
    with pytest.raises(TypeError, match="no CPU path"):
        f.update(object())
    cpu_tracker = type("T", (), dict(tracks_i=torch.zeros((2, 8, 4), dtype=torch.int32), kin=torch.zeros((2, 8, 4), dtype=torch.float64),
                                     stats=torch.zeros((2, 4), dtype=torch.int32)))()
    with pytest.raises(TypeError, match="no CPU path"):
        f.update(cpu_tracker)
    with pytest.raises(ValueError, match="dt"):
        f.tracks(dt=0.0)
    # the session's dict
    assert _filter_kw(None) is None and _filter_kw(False) is None and _filter_kw(True) == {} and _filter_kw(dict(gate=3.0)) == dict(gate=3.0)
    assert _track_kw(dict(filter=True)) == dict(filter=True) and _track_kw(dict(reach=2, filter=dict(max_coast=0))) == dict(reach=2, filter=dict(max_coast=0))
    assert _track_kw(dict(filter=None)) == dict(filter=None) and _track_kw(True) == {} and _track_kw(dict(reach=2)) == dict(reach=2)
    assert _objects_kw(dict(track=dict(filter=True))) == dict(track=dict(filter=True))
    with pytest.raises(TypeError, match="unknown entries"):
        _track_kw(dict(filter=dict(gat=1)))
    with pytest.raises(TypeError, match="unknown entries"):
        _track_kw(dict(filtre=True))
    with pytest.raises(TypeError, match="filter must be"):
        _track_kw(dict(filter="yes"))
    with pytest.raises(ValueError, match="gate"):
        _track_kw(dict(filter=dict(gate=-1.0)))
    opt = J.default_opt(height=256, width=256, occ_map_size=64, imgs_per_gpu=1, type="static", split="odometry")
    net = MONO.module_dict["Baseline"](opt).eval()
    with pytest.raises(TypeError, match="unknown entries"):
        PerceptionStream(net, (94, 311), objects=dict(track=dict(filter=dict(gat=1))))
    with pytest.raises(TypeError, match="filter must be"):
        PerceptionStream(net, (94, 311), objects=dict(track=dict(filter=1)))
    with pytest.raises(ValueError, match="max_tracks"):
        PerceptionStream(net, (94, 311), objects=dict(track=dict(reach=2, filter=dict(max_tracks=300))))
    with pytest.raises(ValueError, match="min_hits"):
        PerceptionStream(net, (94, 311), objects=dict(conn=4, track=dict(filter=dict(min_hits=0))))
    for ok in (dict(track=dict(filter=True)), dict(track=dict(reach=2, filter=dict(max_coast=1, gate=3.0))), dict(track=dict(filter=False))):
        with pytest.raises(RuntimeError, match="GPU"):
            PerceptionStream(net, (94, 311), objects=ok)


# ---------------------------------------------------------------------------------------- the reference against hand-worked cases
def _chain(frames, S=4, M=4, max_coast=2, min_hits=3, gate2=25.0, r=1.0, c0=2.0, q=0.0):
    """one camera; frames: per call the objects [(track_id, X, Z)] in object-id order -> per call (slots_i, slots_d, head, obj_slot, fstats)"""
    st = R.zero_state(1, S)
    si, sd, head = st["slots_i"][0], st["slots_d"][0], st["head"][0]
    out = []
    for objs in frames:
        tr, kin, stats = R.frame([objs], M)
        si, sd, head, oslot, fs = R.step_one(tr[0], kin[0], stats[0], si, sd, head, M, S, max_coast, min_hits, F(gate2), F(r), F(c0), F(q))
        out.append((si, sd, head, oslot, fs))
    return out


def test_reference_squares_each_sigma_once():
    g2, r, c0, q = R.squares(2.0, 0.15625, 3.0, 0.5)
    assert (g2, r, c0, q) == (4.0, 0.0244140625, 9.0, 0.25)
    assert R.squares(0.1, 0.1, 0.1, 0.1)[0] == F(0.1) * F(0.1)


def test_reference_birth_then_one_update_worked_by_hand():
    # birth at X = 10 (Z = -3), then a measurement of 14 with r = 1, c0 = 2, q = 0.  X axis: predicted p' = 10, v' = 0,
    # a' = (1 + (0 + 0)) + 2 = 3, b' = 0 + 2 = 2, c' = 2; y = 4, S = 4, K = (0.75, 0.5); p = 13, v = 2; a = 3 - 0.75 * 3 = 0.75,
    # b = 2 - 0.75 * 2 = 0.5, c = 2 - 0.5 * 2 = 1.  Z axis: y = 0: the state stays (-3, 0), the covariance is the same.
    (i0, d0, h0, o0, f0), (i1, d1, h1, o1, f1) = _chain([[(7, 10.0, -3.0)], [(7, 14.0, -3.0)]])
    assert i0.tolist() == [[0, 1, 7, 1, 1, 0, 0, 0]] + [[0] * 8] * 3
    assert d0.tolist() == [[10.0, -3.0, 0.0, 0.0, 1.0, 0.0, 2.0, 1.0, 0.0, 2.0]] + [[0.0] * 10] * 3
    assert h0.tolist() == [1, 1] and o0.tolist() == [0, -1, -1, -1] and f0.tolist() == [1, 0, 0, 0, 0, 1, 0, 0]
    assert i1.tolist() == [[0, 1, 7, 2, 2, 0, 0, 0]] + [[0] * 8] * 3
    assert d1.tolist() == [[13.0, -3.0, 2.0, 0.0, 0.75, 0.5, 1.0, 0.75, 0.5, 1.0]] + [[0.0] * 10] * 3
    assert h1.tolist() == [1, 2] and o1.tolist() == [0, -1, -1, -1] and f1.tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    assert i1.dtype == np.int32 and d1.dtype == np.float64 and o1.dtype == np.int32 and f1.dtype == np.int32 and h1.dtype == np.int32


def test_reference_process_noise_enters_the_prediction():
    # q = 4 (accel_sigma 2): a' = 3 + 1 = 4, b' = 2 + 2 = 4, c' = 2 + 4 = 6; y = 4, S = 5, K = (0.8, 0.8) -- 4 / 5 in float64
    k = 4.0 / 5.0
    _, (i1, d1, _, _, _) = _chain([[(7, 10.0, -3.0)], [(7, 14.0, -3.0)]], q=4.0)
    assert d1[0, [0, 2, 4, 5, 6]].tolist() == [10.0 + k * 4.0, k * 4.0, 4.0 - k * 4.0, 4.0 - k * 4.0, 6.0 - k * 4.0]


def test_reference_life_cycle_tentative_to_confirmed_at_min_hits():
    # the third measurement, 17 = where the second left it heading (13 + 2 = 15 predicted; a' = (0.75 + 1) + 1 = 2.75, b' = 1.5, c' = 1)
    res = _chain([[(7, 10.0, -3.0)], [(7, 14.0, -3.0)], [(7, 17.0, -3.0)], [(7, 20.0, -3.0)]])
    assert [x[0][0, 1] for x in res] == [1, 1, 2, 2] and [x[0][0, 4] for x in res] == [1, 2, 3, 4] and [x[0][0, 3] for x in res] == [1, 2, 3, 4]
    assert [x[4].tolist()[:3] for x in res] == [[1, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 0]]
    k1, k2 = 2.75 / 3.75, 1.5 / 3.75
    assert res[2][1][0, [0, 2, 4, 5, 6]].tolist() == [15.0 + k1 * 2.0, 2.0 + k2 * 2.0, 2.75 - k1 * 2.75, 1.5 - k1 * 1.5, 1.0 - k2 * 1.5]
    assert [x[0][0, 1] for x in _chain([[(7, 10.0, -3.0)], [(7, 14.0, -3.0)]], min_hits=1)] == [2, 2]
    assert [x[0][0, 1] for x in _chain([[(7, 10.0, -3.0)], [(7, 14.0, -3.0)]], min_hits=2)] == [1, 2]


def test_reference_a_miss_frees_a_tentative_slot():
    res = _chain([[(7, 10.0, -3.0)], [(7, 14.0, -3.0)], [], [(8, 14.0, -3.0)]])
    i2, d2, h2, o2, f2 = res[2]
    assert not i2.any() and not d2.any() and h2.tolist() == [1, 3] and o2.tolist() == [-1] * 4 and f2.tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
    assert res[3][0][0].tolist() == [1, 1, 8, 1, 1, 0, 0, 0] and res[3][2].tolist() == [2, 4]        # a new fid: nothing was kept


def test_reference_coasting_for_max_coast_frames_then_the_end():
    # confirmed standing at X = 10 (every y is 0: the state stays (10, 0)), then no object.  max_coast 2: two coasting frames with the
    # predicted state, the third miss ends the track.  Covariance after three hits at q = 0: worked through the same formulas
    hits = [[(7, 10.0, -3.0)]] * 3
    res = _chain(hits + [[], [], [], []])
    a, b, c = res[2][1][0, 4:7].tolist()
    i3, d3, _, o3, f3 = res[3]
    assert i3[0].tolist() == [0, 3, 7, 4, 3, 1, -1, 0] and f3.tolist() == [1, 0, 1, 0, 0, 0, 0, 0] and o3.tolist() == [-1] * 4
    assert d3[0, [0, 2]].tolist() == [10.0, 0.0] and d3[0, 4:7].tolist() == [(a + (b + b)) + c, b + c, c]
    assert res[4][0][0].tolist() == [0, 3, 7, 5, 3, 2, -1, 0] and res[4][4].tolist() == [1, 0, 1, 0, 0, 0, 0, 0]
    assert not res[5][0].any() and not res[5][1].any() and res[5][4].tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
    assert res[6][4].tolist() == [0] * 8 and res[6][2].tolist() == [1, 7]
    # a moving track coasts along its velocity: after (10, 14, 17) the state is (p, v); one miss -> (p + v, v)
    res = _chain([[(7, 10.0, -3.0)], [(7, 14.0, -3.0)], [(7, 17.0, -3.0)], []])
    p, v = res[2][1][0, [0, 2]].tolist()
    assert res[3][1][0, [0, 2]].tolist() == [p + v, v] and res[3][0][0, 1] == 3
    # max_coast 0: a confirmed track ends at its first miss
    res = _chain(hits + [[]], max_coast=0)
    assert not res[3][0].any() and res[3][4].tolist() == [0, 0, 0, 0, 0, 0, 1, 0]
    # the object comes back in the second coasting frame under a new tracker id: the same fid, confirmed again, misses 0
    res = _chain(hits + [[], [], [(9, 11.0, -3.0)]])
    assert res[5][0][0].tolist() == [0, 2, 9, 6, 4, 0, 0, 0] and res[5][4].tolist() == [1, 1, 0, 0, 1, 0, 0, 0] and res[5][3].tolist() == [0, -1, -1, -1]


def test_reference_reacquire_keeps_the_fid_and_rebinds_src_track():
    # the tracker switches the id 7 -> 9 while the object moves one metre: d2 = 1 <= 25: the slot goes on (the id-switch repair)
    hits = [[(7, 10.0, -3.0)]] * 3
    res = _chain(hits + [[(9, 11.0, -3.0)], [(9, 12.0, -3.0)]])
    assert res[3][0][0].tolist() == [0, 2, 9, 4, 4, 0, 0, 0] and res[3][4].tolist() == [1, 1, 0, 0, 1, 0, 0, 0] and res[3][2].tolist() == [1, 4]
    assert res[4][0][0].tolist() == [0, 2, 9, 5, 5, 0, 0, 0] and res[4][4].tolist() == [1, 1, 0, 1, 0, 0, 0, 0]      # continued under the new id
    # ... and 20 m away (d2 = 400 > 25) it is a birth into slot 1 with fid 1, while slot 0 coasts
    res = _chain(hits + [[(9, 30.0, -3.0)]])
    assert res[3][0][:2].tolist() == [[0, 3, 7, 4, 3, 1, -1, 0], [1, 1, 9, 1, 1, 0, 0, 0]]
    assert res[3][4].tolist() == [2, 0, 1, 0, 0, 1, 0, 0] and res[3][3].tolist() == [1, -1, -1, -1] and res[3][2].tolist() == [2, 4]
    # exactly on the gate (d2 = 25 <= 25) qualifies; gate 0 admits only d2 = 0
    assert _chain(hits + [[(9, 13.0, 1.0)]])[3][4].tolist() == [1, 1, 0, 0, 1, 0, 0, 0]
    assert _chain(hits + [[(9, 10.0, -3.0)]], gate2=0.0)[3][4].tolist() == [1, 1, 0, 0, 1, 0, 0, 0]
    assert _chain(hits + [[(9, 10.0, -2.5)]], gate2=0.0)[3][4].tolist() == [2, 0, 1, 0, 0, 1, 0, 0]
    # the distance is taken from the PREDICTED position: a track at 17 moving about 2.5 m a frame is found again near 19.5, not at 17
    mov = [[(7, 10.0, -3.0)], [(7, 14.0, -3.0)], [(7, 17.0, -3.0)]]
    p, v = _chain(mov)[2][1][0, [0, 2]].tolist()
    assert _chain(mov + [[(9, p + v + 0.5, -3.0)]], gate2=1.0)[3][4][4] == 1 and _chain(mov + [[(9, p, -3.0)]], gate2=1.0)[3][4][4] == 0


def test_reference_equidistant_tie_goes_to_the_smaller_slot_then_the_smaller_object():
    # two confirmed slots at X = -2 and X = +2 (fids 0, 1), one object with a new id at 0: d2 = 4 for both, bit-equal: slot 0 takes it
    two = [[(1, -2.0, 0.0), (2, 2.0, 0.0)]] * 3
    res = _chain(two + [[(5, 0.0, 0.0)]])
    assert res[3][0][:2, [0, 1, 2, 5, 6]].tolist() == [[0, 2, 5, 0, 0], [1, 3, 2, 1, -1]] and res[3][3].tolist() == [0, -1, -1, -1]
    assert res[3][4].tolist() == [2, 1, 1, 0, 1, 0, 0, 0]
    # by slot index, not by position: with the slots the other way round it is still slot 0
    res = _chain([[(1, 2.0, 0.0), (2, -2.0, 0.0)]] * 3 + [[(5, 0.0, 0.0)]])
    assert res[3][0][:2, [0, 1, 2]].tolist() == [[0, 2, 5], [1, 3, 2]]
    # one slot at 0, two new objects at +2 (id 0) and -2 (id 1): object 0 is taken, object 1 is born
    res = _chain([[(1, 0.0, 0.0)]] * 3 + [[(5, 2.0, 0.0), (6, -2.0, 0.0)]])
    assert res[3][0][:2, [0, 1, 2, 6]].tolist() == [[0, 2, 5, 0], [1, 1, 6, 1]] and res[3][3].tolist() == [0, 1, -1, -1]
    assert res[3][4].tolist() == [2, 1, 0, 0, 1, 1, 0, 0]
    # greedy takes the nearest pair first: slots at 0 and 3, objects at 2 and 5 -> (slot 1, object 0) d2 = 1 first, then nothing is
    # left for slot 0 within gate 2.5 (d2 = 25 > 6.25) although object 0 was within its gate
    res = _chain([[(1, 0.0, 0.0), (2, 3.0, 0.0)]] * 3 + [[(5, 2.0, 0.0), (6, 5.0, 0.0)]], gate2=6.25)
    assert res[3][3].tolist() == [1, 2, -1, -1] and res[3][0][:3, [0, 1, 2]].tolist() == [[0, 3, 1], [1, 2, 5], [2, 1, 6]]


def test_reference_slot_exhaustion_counts_dropped_and_a_freed_slot_waits_for_the_next_call():
    # two slots, three objects: the third finds no slot and takes no fid
    res = _chain([[(1, 0.0, 0.0), (2, 10.0, 0.0), (3, 20.0, 0.0)]], S=2)
    assert res[0][4].tolist() == [2, 0, 0, 0, 0, 2, 0, 1] and res[0][2].tolist() == [2, 1] and res[0][3].tolist() == [0, 1, -1, -1]
    # slot 0 (tentative, track 1) is missed and freed in the second call, but it was not free at entry: object 1 (track 3, 20 m from
    # everything) is dropped there and born into slot 0 in the third call, with the next fid
    res = _chain([[(1, 0.0, 0.0), (2, 10.0, 0.0)], [(2, 10.0, 0.0), (3, 20.0, 0.0)], [(2, 10.0, 0.0), (3, 20.0, 0.0)]], S=2)
    assert res[1][4].tolist() == [1, 0, 0, 1, 0, 0, 1, 1] and res[1][3].tolist() == [1, -1, -1, -1] and res[1][2].tolist() == [2, 2]
    assert not res[1][0][0].any() and res[1][0][1, [0, 1, 4, 6]].tolist() == [1, 1, 2, 0]
    assert res[2][4].tolist() == [2, 1, 0, 1, 0, 1, 0, 0] and res[2][3].tolist() == [1, 0, -1, -1] and res[2][2].tolist() == [3, 3]
    assert res[2][0][0].tolist() == [2, 1, 3, 1, 1, 0, 1, 0]


def test_reference_non_finite_measurements_are_ignored():
    hits = [[(7, 10.0, -3.0)]] * 3
    for bad in ((float("nan"), -3.0), (10.0, float("inf")), (-float("inf"), float("nan"))):
        res = _chain(hits + [[(7,) + bad, (8,) + bad]])
        i3, d3, h3, o3, f3 = res[3]
        assert i3[0].tolist() == [0, 3, 7, 4, 3, 1, -1, 0] and not i3[1:].any() and np.isfinite(d3).all()
        assert o3.tolist() == [-1] * 4 and f3.tolist() == [1, 0, 1, 0, 0, 0, 0, 0] and h3.tolist() == [1, 4]
    # a valid object next to an invalid one is handled as if it were alone
    res = _chain(hits + [[(7, float("nan"), 0.0), (9, 10.5, -3.0)]])
    assert res[3][3].tolist() == [-1, 0, -1, -1] and res[3][0][0].tolist() == [0, 2, 9, 4, 4, 0, 1, 0] and np.isfinite(res[3][1]).all()


def test_reference_clamps_the_count_and_never_indexes_with_a_track_id():
    tr, kin, stats = R.frame([[(2 ** 31 - 1, 1.0, 2.0), (-5, 3.0, 4.0)]], 2)
    z = R.zero_state(1, 4)
    for count, want in ((-7, [0, 0]), (0, [0, 0]), (1, [1, 0]), (2, [2, 0]), (3, [2, 0]), (2 ** 31 - 1, [2, 0])):
        stats[0, 0] = count
        o, f, new = R.step(tr, kin, stats, z, 2, 4, meas_sigma=1.0)
        assert f[0, [5, 7]].tolist() == want and new["head"][0].tolist() == [want[0], 1]
    assert new["slots_i"][0, :2, 2].tolist() == [2 ** 31 - 1, -5] and not z["slots_i"].any()        # the state handed in is left as it was
