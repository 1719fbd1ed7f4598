"""dw of every case of tests/wgrad_route_cases.py under two builds of the library, byte for byte: needs a GPU.

    python tools/wgrad_dw_ab.py <libjperceiver_hip.so A> <libjperceiver_hip.so B>

Each library runs the cases in a process of its own (JP_LIB_PATH is read at load time): dw written (accumulate = 0), then added onto
that result (accumulate = 1), SHA-256 of the bytes.  The cases of BITWISE sum every partial result through scratch in a fixed order:
two builds that differ in host code only must agree on them exactly, and a fold that changed its kernel or its order shows here
although it stays inside the tolerance of tests/test_wgrad_routes_gpu.py.  The atomic-epilogue cases are listed, not held.
Exit status 1 when a BITWISE case differs."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump():
    import torch
    from tests import wgrad_route_cases as C, test_wgrad_routes_gpu as T
    out = {}
    for case in C.CASES + C.DIRECT_CASES:
        xs, dy = T._operands(case)
        dw = torch.zeros(case[2], sum(c for c, _ in case[1]), case[6], case[6], device=dy.device)
        sha = []
        for accumulate in (0, 1):
            T._wgrad(case, xs, dy, dw, accumulate)
            torch.cuda.synchronize()
            sha.append(hashlib.sha256(dw.cpu().numpy().tobytes()).hexdigest())
        out[case[0]] = sha
    print(json.dumps(out))


def main(a, b):
    from tests import wgrad_route_cases as C
    res = []
    for lib in (a, b):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--dump"], env=dict(os.environ, JP_LIB_PATH=os.path.abspath(lib)),
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f"{lib}: the dump failed (status {r.returncode})\n{r.stderr[-2000:]}")
        res.append(json.loads(r.stdout.splitlines()[-1]))
    bad = 0
    for label in res[0]:
        same, held = res[0][label] == res[1][label], label in C.BITWISE
        bad += held and not same
        print(f"{'same' if same else 'DIFFERENT':9s} {'bitwise' if held else 'atomic/direct':13s} {label}")
    print(f"{bad} differences among the {len(C.BITWISE)} bitwise cases")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1:] == ["--dump"]:
        dump()
    elif len(sys.argv) == 3:
        sys.exit(main(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
