"""Plain numpy / Python restatement of jp_bev_track_filter (csrc/bevfilter.hip) for the tests: the header's sequential definition step by
step -- loops over the slots and the objects, a sequential greedy loop over all pairs -- with the float64 arithmetic one operation per
line in the header's order (np.float64 scalars: every operation is rounded once).  It shares no code with the package.  State and
outputs have the layouts the header gives them."""
import numpy as np

F = np.float64
FREE, TENTATIVE, CONFIRMED, COASTING = 0, 1, 2, 3


def zero_state(B, S):
    """no history"""
    return {"slots_i": np.zeros((B, S, 8), dtype=np.int32), "slots_d": np.zeros((B, S, 10), dtype=np.float64),
            "head": np.zeros((B, 2), dtype=np.int32)}


def squares(gate, meas_sigma, vel_sigma0, accel_sigma):
    """each squared once, one rounded multiply -> gate2, r, c0, q"""
    return F(gate) * F(gate), F(meas_sigma) * F(meas_sigma), F(vel_sigma0) * F(vel_sigma0), F(accel_sigma) * F(accel_sigma)


def predict_axis(p, v, a, b, c, q):
    p = p + v
    t = b + b
    t = a + t
    t = t + c
    a2 = t + q * F(0.25)                                                # q / 4: a power of two, the same rounding
    t = b + c
    b2 = t + q * F(0.5)
    c2 = c + q
    return p, v, a2, b2, c2


def update_axis(p, v, a, b, c, z, r):
    y = z - p
    s = a + r
    k1 = a / s
    k2 = b / s
    t = k1 * y
    p2 = p + t
    t = k2 * y
    v2 = v + t
    t = k1 * a
    a2 = a - t
    t = k1 * b
    b2 = b - t
    t = k2 * b
    c2 = c - t
    return p2, v2, a2, b2, c2


def step_one(tracks, kin, stats, slots_i, slots_d, head, M, S, max_coast, min_hits, gate2, r, c0, q):
    """one camera, one call -> the new slots_i (S, 8), slots_d (S, 10), head (2), obj_slot (M), fstats (8)"""
    si = [[int(x) for x in row] for row in slots_i]
    sd = [[F(x) for x in row] for row in slots_d]
    next_fid, calls = int(head[0]), int(head[1])
    # 0. the objects
    n = min(max(int(stats[0]), 0), M)
    t = [int(tracks[c][0]) for c in range(n)]
    z = [(F(kin[c][0]), F(kin[c][1])) for c in range(n)]
    valid = [bool(np.isfinite(z[c][0]) and np.isfinite(z[c][1])) for c in range(n)]
    live = [1 <= si[s][1] <= 3 for s in range(S)]
    free_at_entry = [s for s in range(S) if not live[s]]
    # 1. predict
    for s in range(S):
        if live[s]:
            d = sd[s]
            d[0], d[2], d[4], d[5], d[6] = predict_axis(d[0], d[2], d[4], d[5], d[6], q)
            d[1], d[3], d[7], d[8], d[9] = predict_axis(d[1], d[3], d[7], d[8], d[9], q)
    slot_obj, obj_slot = {}, {}                                         # slot -> the object it takes, and back
    # 2. continue (a slot picks the smallest valid object with its src_track; the object goes to the smallest slot that picked it)
    continued = 0
    for s in range(S):
        if not (live[s] and si[s][5] == 0):
            continue
        for c in range(n):
            if valid[c] and t[c] == si[s][2]:
                if c not in obj_slot:
                    slot_obj[s], obj_slot[c] = c, s
                    continued += 1
                break
    # 3. re-acquire: all qualifying pairs, then greedily the smallest (d2, slot, object)
    pairs = []
    for s in range(S):
        if not live[s] or s in slot_obj:
            continue
        for c in range(n):
            if not valid[c] or c in obj_slot:
                continue
            dx = z[c][0] - sd[s][0]
            dz = z[c][1] - sd[s][1]
            a = dx * dx
            b = dz * dz
            d2 = a + b
            if d2 <= gate2:                                             # False for NaN
                pairs.append((d2, s, c))
    pairs.sort()
    reacquired = 0
    for d2, s, c in pairs:
        if s in slot_obj or c in obj_slot:
            continue
        slot_obj[s], obj_slot[c] = c, s
        si[s][2] = t[c]
        reacquired += 1
    # 4. births
    born = dropped = 0
    births = []
    for c in range(n):
        if not valid[c] or c in obj_slot:
            continue
        if born < len(free_at_entry):
            s = free_at_entry[born]
            si[s] = [next_fid, 0, t[c], 1, 1, 0, c, 0]
            sd[s] = [z[c][0], z[c][1], F(0), F(0), r, F(0), c0, r, F(0), c0]
            next_fid += 1
            born += 1
            slot_obj[s], obj_slot[c] = c, s
            births.append(s)
        else:
            dropped += 1
    # 5. update, 6. miss
    ended = 0
    for s in range(S):
        if not live[s]:
            continue
        if s in slot_obj:
            c, d = slot_obj[s], sd[s]
            d[0], d[2], d[4], d[5], d[6] = update_axis(d[0], d[2], d[4], d[5], d[6], z[c][0], r)
            d[1], d[3], d[7], d[8], d[9] = update_axis(d[1], d[3], d[7], d[8], d[9], z[c][1], r)
            si[s][3] += 1
            si[s][4] += 1
            si[s][5] = 0
            si[s][6] = c
        elif si[s][1] == TENTATIVE or si[s][5] + 1 > max_coast:
            si[s], sd[s] = [0] * 8, [F(0)] * 10
            ended += 1
        else:
            si[s][5] += 1
            si[s][3] += 1
            si[s][1] = COASTING
            si[s][6] = -1
    # 7. status of the slots with a measurement; a slot that is not live at exit is zero
    for s in slot_obj:
        si[s][1] = CONFIRMED if si[s][4] >= min_hits else TENTATIVE
        si[s][7] = 0
    for s in range(S):
        if not 1 <= si[s][1] <= 3:
            si[s], sd[s] = [0] * 8, [F(0)] * 10
    status = [si[s][1] for s in range(S)]
    fstats = [sum(1 for x in status if x != 0), status.count(CONFIRMED), status.count(COASTING), continued, reacquired, born, ended, dropped]
    out_slot = np.full((M,), -1, dtype=np.int32)
    for c, s in obj_slot.items():
        out_slot[c] = s
    return (np.array(si, dtype=np.int32).reshape(S, 8), np.array(sd, dtype=np.float64).reshape(S, 10),
            np.array([next_fid, calls + 1], dtype=np.int32), out_slot, np.array(fstats, dtype=np.int32))


def step(tracks, kin, stats, state, M, S, max_coast=3, min_hits=3, gate=2.0, meas_sigma=1.0, vel_sigma0=3.0, accel_sigma=0.5):
    """tracks (B, M, 4) int32, kin (B, M, 4) float64, stats (B, 4) int32 as jp_bev_tracks writes them; state: zero_state's dict (left
    unchanged) -> obj_slot (B, M), fstats (B, 8), the new state"""
    gate2, r, c0, q = squares(gate, meas_sigma, vel_sigma0, accel_sigma)
    with np.errstate(all="ignore"):
        res = [step_one(tracks[b], kin[b], stats[b], state["slots_i"][b], state["slots_d"][b], state["head"][b], M, S, max_coast, min_hits,
                        gate2, r, c0, q) for b in range(tracks.shape[0])]
    new = {"slots_i": np.stack([x[0] for x in res]), "slots_d": np.stack([x[1] for x in res]), "head": np.stack([x[2] for x in res])}
    return np.stack([x[3] for x in res]), np.stack([x[4] for x in res]), new


# ---------------------------------------------------------------------------------------- inputs shared by the tests
def frame(objs, M, B=None):
    """objs: per camera a list of (track_id, X, Z) in object-id order -> tracks, kin, stats with jp_bev_tracks' layouts (the fields the
    filter does not read are filled like the tracker's: age 1, prev -1, overlap 0, zero displacements)"""
    B = len(objs) if B is None else B
    tracks = np.tile(np.array([-1, 0, -1, 0], dtype=np.int32), (B, M, 1))
    kin = np.zeros((B, M, 4), dtype=np.float64)
    stats = np.zeros((B, 4), dtype=np.int32)
    for b, rows in enumerate(objs):
        stats[b, 0] = len(rows)
        for c, (tid, X, Z) in enumerate(rows):
            tracks[b, c] = [tid, 1, -1, 0]
            kin[b, c, :2] = [X, Z]
    return tracks, kin, stats
