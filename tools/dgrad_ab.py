"""The input gradient of two builds of the library, side by side.

    python tools/dgrad_ab.py queries <libjperceiver_hip.so A> <libjperceiver_hip.so B>      (needs no GPU)
    python tools/dgrad_ab.py dx <libjperceiver_hip.so A> <libjperceiver_hip.so B>           (needs a GPU)

queries: jp_conv2d_dgrad_split_floats and jp_conv2d_ws_floats(.., 1) over the shape grid of tools/wgrad_query_ab.py,
jp_conv2d_dgrad_src3_split_floats and jp_conv2d_dgrad_src3_ok over the source lists of tests/conv_route_cases.py,
tests/wgrad_route_cases.py and tests/dgrad_route_cases.py.  ops.conv2d allocates by these answers and picks the entry point by the
last, so a change that only moves host code must print `0 differences`.

dx: every case of tests/dgrad_route_cases.py under each library, in a process of its own per library (JP_LIB_PATH is read at load
time): dx written (accumulate = 0), replayed from the pack that call left (ws_state = 1), and added onto the first result
(accumulate = 1); SHA-256 of the bytes of every source's dx, and the pack scratch saved.  Then the packs are crossed: a third and a
fourth process replay, with ws_state = 1, the pack the OTHER library built.  Every case outside ATOMIC must give the same bytes in
all of these; the atomic ones are listed, not held.  Exit status 1 otherwise."""
import ctypes
import hashlib
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def source_lists():
    from tests import conv_route_cases as A, wgrad_route_cases as B, dgrad_route_cases as D
    from tools.wgrad_query_ab import COUTS
    seen, couts = [], set(COUTS)
    rows = [(c[0], c[1]) for c in A.ROUTE_CASES + A.GPU_ROUTE_CASES] + [(c[1], c[2]) for c in B.CASES + B.DIRECT_CASES + D.CASES]
    for srcs, cout in rows:
        key = tuple(D.cu6(srcs))
        if key not in seen:
            seen.append(key)
        couts.add(cout)
    return seen, sorted(couts)


def queries(a, b):
    from tools.wgrad_query_ab import CINS, COUTS, MAPS, NS, KSP
    libs = [ctypes.CDLL(os.path.abspath(p)) for p in (a, b)]
    for L in libs:
        for name, nargs in (("jp_conv2d_dgrad_split_floats", 8), ("jp_conv2d_dgrad_src3_split_floats", 9), ("jp_conv2d_ws_floats", 4)):
            getattr(L, name).restype, getattr(L, name).argtypes = ctypes.c_long, [ctypes.c_int] * nargs
        L.jp_conv2d_dgrad_src3_ok.restype, L.jp_conv2d_dgrad_src3_ok.argtypes = ctypes.c_int, [ctypes.c_int] * 14
    n = bad = 0

    def both(name, *args):
        nonlocal n, bad
        n += 1
        ra, rb = getattr(libs[0], name)(*args), getattr(libs[1], name)(*args)
        if ra != rb:
            bad += 1
            print(f"{name}{args}: {ra} vs {rb}")

    for N, cin, (H, W), cout, (K, s, p) in itertools.product(NS, CINS, MAPS, COUTS, KSP):
        both("jp_conv2d_dgrad_split_floats", N, cin, H, W, cout, K, s, p)
    for cin, cout, (K, s, p) in itertools.product(CINS, COUTS, KSP):
        both("jp_conv2d_ws_floats", cin, cout, K, 1)
    lists, couts = source_lists()
    for key, N, (H, W) in itertools.product(lists, NS, MAPS):
        both("jp_conv2d_dgrad_src3_split_floats", *key, N, H, W)
    for key, cout, N, (H, W), (K, s, p), pm in itertools.product(lists, couts, NS, MAPS + ((128, 384), (192, 256)), KSP, (0, 1)):
        both("jp_conv2d_dgrad_src3_ok", *key, N, H, W, cout, K, s, p, pm)
    print(f"{n} calls over {len(lists)} source lists")
    print(f"{bad} differences")
    return 1 if bad else 0


def _sha(ts):
    import torch
    torch.cuda.synchronize()
    return [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in ts]


def dump(save_dir, load_dir):
    """load_dir empty: run every case, save its pack; else: replay the packs found there"""
    import torch
    from tests import dgrad_route_cases as C, test_dgrad_routes_gpu as T
    out = {}
    for k, case in enumerate(C.CASES):
        w, dy = T._operands(case)
        shapes = [(case[3], c, case[4] >> u, case[5] >> u) for c, u in case[1]]
        fresh = lambda: [torch.full(s, float("nan"), device=dy.device) for s in shapes]         # noqa: E731
        if load_dir:
            if not case[10]:
                continue
            ws = torch.load(os.path.join(load_dir, f"{k}.pt")).to(dy.device)
            dxs = fresh()
            T.run_case(case, w, dy, dxs, 0, ws, 1)
            out[case[0]] = {"crossed": _sha(dxs)}
            continue
        ws = T.pack_scratch(case, dy.device)
        dxs = fresh()
        T.run_case(case, w, dy, dxs, 0, ws, 0)
        res = {"written": _sha(dxs)}
        if ws is not None:
            torch.save(ws.cpu(), os.path.join(save_dir, f"{k}.pt"))
            again = fresh()
            T.run_case(case, w, dy, again, 0, ws, 1)
            res["replayed"] = _sha(again)
        T.run_case(case, w, dy, dxs, 1, ws, 1 if ws is not None else 0)
        res["accumulated"] = _sha(dxs)
        out[case[0]] = res
    print(json.dumps(out))


def _child(lib, save_dir, load_dir):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", save_dir, load_dir],
                       env=dict(os.environ, JP_LIB_PATH=os.path.abspath(lib)), capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f"{lib}: the dump failed (status {r.returncode})\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.splitlines()[-1])


def dx(a, b):
    from tests import dgrad_route_cases as C
    with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
        own = [_child(a, da, ""), _child(b, db, "")]
        crossed = [_child(a, "", db), _child(b, "", da)]      # A replays B's packs, B replays A's
    bad = 0
    for case in C.CASES:
        label = case[0]
        ra, rb = own[0][label], own[1][label]
        same = ra == rb
        if label in crossed[0]:
            same = same and crossed[0][label]["crossed"] == crossed[1][label]["crossed"] == ra["written"] == ra["replayed"]
        held = label not in C.ATOMIC
        bad += held and not same
        print(f"{'same' if same else 'DIFFERENT':9s} {'bitwise' if held else 'atomic':7s} {label}")
    print(f"{bad} differences among the {len(C.CASES) - len(C.ATOMIC)} bitwise cases")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] in ("queries", "dx"):
        sys.exit({"queries": queries, "dx": dx}[sys.argv[1]](sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
