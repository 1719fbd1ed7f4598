"""The weight-gradient scratch queries of two builds of the library, side by side: needs no GPU.

    python tools/wgrad_query_ab.py <libjperceiver_hip.so A> <libjperceiver_hip.so B>

jp_conv2d_wgrad_ws_floats over a grid of layer shapes and jp_conv2d_wgrad_src3_ws_floats over the source lists of
tests/conv_route_cases.py and tests/wgrad_route_cases.py, at both pad modes.  ops.conv2d allocates the scratch by these answers and the
split counts follow from the scratch, so a change that only moves host code must print `0 differences`.  Exit status 1 otherwise."""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CINS = (1, 3, 6, 8, 16, 32, 40, 64, 65, 96, 128, 129, 160, 192, 256, 257, 512, 513)
COUTS = (1, 2, 8, 16, 24, 48, 64, 68, 72, 128, 192, 256, 512)
MAPS = ((4, 4), (6, 96), (8, 24), (8, 64), (16, 64), (16, 128), (32, 32), (64, 256), (192, 640), (256, 256))
NS = (1, 2, 8, 16)
KSP = ((1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1), (7, 2, 3))


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    one, src3 = lib.jp_conv2d_wgrad_ws_floats, lib.jp_conv2d_wgrad_src3_ws_floats
    one.restype = src3.restype = ctypes.c_long
    one.argtypes = [ctypes.c_int] * 8
    src3.argtypes = [ctypes.c_int] * 14
    return one, src3


def source_lists():
    from tests import conv_route_cases as A, wgrad_route_cases as B
    seen, couts = [], set(COUTS)
    for srcs, cout in [(c[0], c[1]) for c in A.ROUTE_CASES + A.GPU_ROUTE_CASES] + [(c[1], c[2]) for c in B.CASES + B.DIRECT_CASES]:
        flat = [a for cu in srcs for a in cu]
        key = tuple(flat + [0] * (6 - len(flat)))
        if key not in seen:
            seen.append(key)
        couts.add(cout)
    return seen, sorted(couts)


def main(a, b):
    (one_a, src3_a), (one_b, src3_b) = load(a), load(b)
    n = bad = 0
    for N, cin, (H, W), cout, (K, s, p) in itertools.product(NS, CINS, MAPS, COUTS, KSP):
        n += 1
        ra, rb = one_a(N, cin, H, W, cout, K, s, p), one_b(N, cin, H, W, cout, K, s, p)
        if ra != rb:
            bad += 1
            print(f"jp_conv2d_wgrad_ws_floats(N={N}, Cin={cin}, H={H}, W={W}, Cout={cout}, K={K}, s={s}, p={p}): {ra} vs {rb}")
    print(f"jp_conv2d_wgrad_ws_floats: {n} calls")
    m = 0
    lists, couts = source_lists()
    for key, cout, N, (H, W), (K, s, p), pm in itertools.product(lists, couts, NS, MAPS, KSP, (0, 1)):
        m += 1
        args = key + (N, H, W, cout, K, s, p, pm)
        ra, rb = src3_a(*args), src3_b(*args)
        if ra != rb:
            bad += 1
            print(f"jp_conv2d_wgrad_src3_ws_floats{args}: {ra} vs {rb}")
    print(f"jp_conv2d_wgrad_src3_ws_floats: {m} calls over {len(lists)} source lists")
    print(f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
