"""Float64 references of the BEV-layout head's dense algebra (jperceiver_amd/csrc/small.hip and the three kernels of pointwise.hip
that only that head uses), written from the formulas in torch float64 on the CPU.  Nothing here calls the oracle or the HIP library.
tests/test_dense_ref_cpu.py holds every function to torch's (or the oracle's) float64 evaluation of the same operation.

Every sum also returns the sum of the magnitudes of its terms: the scale of the per-element error metric of tests/dense_cases.py.
The functions the two chains use are plain differentiable torch expressions, so that autograd in float64 gives their gradients."""
import torch

F64 = torch.float64
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------- strided-batched GEMM
def gemm_operands(A, B, M, N, K, lda, ldb, sA, sB, batch, tA, tB):
    """the (batch, M, K) and (batch, K, N) operands that jp_gemm_strided_batched reads out of the flat buffers A and B:
    op(A)[b][m][k] = A[b sA + (k lda + m  if tA else  m lda + k)],  op(B)[b][k][n] = B[b sB + (n ldb + k  if tB else  k ldb + n)]"""
    b = torch.arange(batch).view(-1, 1, 1)
    m, k = torch.arange(M).view(1, -1, 1), torch.arange(K).view(1, 1, -1)
    ia = b * sA + (k * lda + m if tA else m * lda + k)
    k, n = torch.arange(K).view(1, -1, 1), torch.arange(N).view(1, 1, -1)
    ib = b * sB + (n * ldb + k if tB else k * ldb + n)
    return A[ia], B[ib]


def gemm_c_index(M, N, ldc, sC, batch):
    return torch.arange(batch).view(-1, 1, 1) * sC + torch.arange(M).view(1, -1, 1) * ldc + torch.arange(N).view(1, 1, -1)


def gemm(A, B, C, M, N, K, lda, ldb, ldc, sA, sB, sC, batch, tA, tB, alpha, beta):
    """C[b] = alpha op(A[b]) op(B[b]) + beta C[b] on flat float64 buffers -> (the new flat C, |terms| per written element (batch, M, N)).
    beta == 0 does not read C (whatever it holds, a NaN included, is overwritten); elements of C outside the M x N extents (padding
    columns of ldc > N) keep their value"""
    a, b = gemm_operands(A.double(), B.double(), M, N, K, lda, ldb, sA, sB, batch, tA, tB)
    prod = torch.zeros(batch, M, N, dtype=F64)
    mag = torch.zeros(batch, M, N, dtype=F64)
    for k in range(K):                                   # sum_k a[m][k] b[k][n], term by term
        t = a[:, :, k:k + 1] * b[:, k:k + 1, :]
        prod += t
        mag += t.abs()
    ic = gemm_c_index(M, N, ldc, sC, batch)
    out = C.double().clone()
    old = out[ic]
    if beta != 0:
        out[ic] = alpha * prod + beta * old
        mag = abs(alpha) * mag + (beta * old).abs()
    else:
        out[ic] = alpha * prod
        mag = abs(alpha) * mag
    return out, mag


# ------------------------------------------------------------------------------------------- rows: bias, activation, column sum
def act(pre, kind, gate=None):
    """gate: the (pre > 0) decision to use for relu / leaky relu (default: the reference's own)"""
    if kind == ACT_NONE:
        return pre
    if kind == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-pre))
    g = (pre > 0) if gate is None else gate
    return torch.where(g, pre, pre * (0.0 if kind == ACT_RELU else 0.01))


def bias_act_rows(y, bias, kind):
    """act(y[r][c] + bias[c]) -> (value, pre-activation, |y| + |bias|)"""
    y = y.double()
    b = torch.zeros(y.shape[-1], dtype=F64) if bias is None else bias.double()
    pre = y + b
    return act(pre, kind), pre, y.abs() + b.abs()


def colsum(x, out0=None):
    """out[c] = (out0[c] +) sum_r x[r][c] -> (value, sum of |terms|)"""
    x = x.double()
    s, mag = x.sum(0), x.abs().sum(0)
    if out0 is not None:
        s, mag = s + out0.double(), mag + out0.double().abs()
    return s, mag


def linear(x, w, b):
    """x (..., K) @ w (Nf, K)^T + b: differentiable -> pre-activation"""
    return (x.unsqueeze(-2) * w).sum(-1) + b


def linear_terms(x, w, b):
    return (x.abs().unsqueeze(-2) * w.abs()).sum(-1) + b.abs()


# ------------------------------------------------------------------------------------------- column max, gather
def colmax(E):
    """E (B, R, Cn) -> (value (B, Cn), index (B, Cn) int64): the FIRST maximal row of every column; a column that holds a NaN gives NaN
    and the row of its first NaN (what torch.max(dim=1) does)"""
    B, R, Cn = E.shape
    val = E[:, 0].clone()
    idx = torch.zeros(B, Cn, dtype=torch.int64)
    for i in range(1, R):
        v = E[:, i]
        take = (v > val) | (torch.isnan(v) & ~torch.isnan(val))
        val = torch.where(take, v, val)
        idx = torch.where(take, torch.full_like(idx, i), idx)
    return val, idx


def colmax_bwd(dval, idx, R):
    """dE[b][i][j] = dval[b][j] where idx[b][j] == i, else 0"""
    rows = torch.arange(R).view(1, R, 1)
    return torch.where(idx.unsqueeze(1) == rows, dval.unsqueeze(1).expand(-1, R, -1), torch.zeros((), dtype=dval.dtype))


def select_rows(E, idx):
    """E[b][idx[b][j]][j]: the column maximum once the index is decided (differentiable in E)"""
    return torch.gather(E, 1, idx.unsqueeze(1)).squeeze(1)


def gather_cols(V, idx):
    """T[b][c][j] = V[b][c][idx[b][j]]   (differentiable in V)"""
    B, C, Nn = V.shape
    b = torch.arange(B).view(B, 1, 1)
    c = torch.arange(C).view(1, C, 1)
    return V[b, c, idx.view(B, 1, Nn)]


def gather_cols_bwd(dT, idx):
    """dV[b][c][i] = sum_{j: idx[b][j] == i} dT[b][c][j] -> (value, sum of |terms|, hit count (B, Nn))"""
    dT = dT.double()
    B, C, Nn = dT.shape
    hit = (idx.view(B, 1, Nn) == torch.arange(Nn).view(1, Nn, 1)).double()          # (B, i, j)
    return torch.einsum("bij,bcj->bci", hit, dT), torch.einsum("bij,bcj->bci", hit, dT.abs()), hit.sum(2)


def rot270_index(n):
    """the index row of net.rot270: out[i][j] = x[n - 1 - j][i], flat"""
    i = torch.arange(n).view(n, 1).expand(n, n)
    j = torch.arange(n).view(1, n).expand(n, n)
    return ((n - 1 - j) * n + i).reshape(-1)


# ------------------------------------------------------------------------------------------- spatial mean
def spatial_mean(x, scale):
    """x (BC, HW) -> (scale * mean over HW, scale / HW * sum |x|)"""
    x = x.double()
    HW = x.shape[1]
    return x.sum(1) * scale / HW, x.abs().sum(1) * abs(scale) / HW


def spatial_mean_bwd(dout, HW, scale):
    return (dout.double() * scale / HW).view(-1, 1).expand(-1, HW)


# ------------------------------------------------------------------------------------------- per-channel n x n product
def bcast_matmul(attn, V):
    """out[b,c,i,j] = sum_k attn[b,i,k] V[b,c,k,j]; attn (B, n, n), V (B, C, n, n)   (differentiable)"""
    return (attn[:, None, :, :, None] * V[:, :, None, :, :]).sum(3)


def bcast_matmul_terms(attn, V):
    return (attn.abs()[:, None, :, :, None] * V.abs()[:, :, None, :, :]).sum(3)


def bcast_matmul_bwd(attn, V, dOut):
    """-> dattn[b,i,k] = sum_c sum_j dOut[b,c,i,j] V[b,c,k,j], its |terms|, dV[b,c,k,j] = sum_i attn[b,i,k] dOut[b,c,i,j], its |terms|"""
    attn, V, dOut = attn.double(), V.double(), dOut.double()
    da = (dOut[:, :, :, None, :] * V[:, :, None, :, :]).sum((1, 4))
    da_mag = (dOut.abs()[:, :, :, None, :] * V.abs()[:, :, None, :, :]).sum((1, 4))
    dv = (attn[:, None, :, :, None] * dOut[:, :, :, None, :]).sum(2)
    dv_mag = (attn.abs()[:, None, :, :, None] * dOut.abs()[:, :, :, None, :]).sum(2)
    return da, da_mag, dv, dv_mag


# ------------------------------------------------------------------------------------------- channel-broadcast product, softmax
def mul_bcast_c(a, s):
    """a (B, C, HW) * s (B, 1, HW)   (differentiable)"""
    return a * s


def mul_bcast_c_bwd_s(dout, a):
    """ds[b][p] = sum_c dout[b][c][p] a[b][c][p] -> (value, sum of |terms|)"""
    t = dout.double() * a.double()
    return t.sum(1), t.abs().sum(1)


def softmax_c2(x):
    """x (N, 2, HW) -> softmax over the two channels, with the maximum subtracted first"""
    x = x.double()
    m = torch.maximum(x[:, 0], x[:, 1])
    e0, e1 = torch.exp(x[:, 0] - m), torch.exp(x[:, 1] - m)
    return torch.stack((e0 / (e0 + e1), e1 / (e0 + e1)), 1)


# ------------------------------------------------------------------------------------------- the two chains
def mlp_chain(x, w1, b1, w2, b2, gates=None):
    """TransformModule: relu(linear(relu(linear(x)))) on x (B, C, H, W) seen as (B, C, HW) rows.  gates: the two (pre > 0) decisions
    to replay (default: the reference's own) -> (y (B, C, H, W), [pre1, pre2], hidden)"""
    B, C, H, W = x.shape
    v = x.reshape(B, C, H * W)
    p1 = linear(v, w1, b1)
    h = act(p1, ACT_RELU, None if gates is None else gates[0])
    p2 = linear(h, w2, b2)
    y = act(p2, ACT_RELU, None if gates is None else gates[1])
    return y.reshape(B, C, H, W), [p1, p2], h


def energy(k, q):
    """E[b][i][j] = sum_c k[b][c][i] q[b][c][j]   (differentiable)"""
    return (k[:, :, :, None] * q[:, :, None, :]).sum(1)


def energy_terms(k, q):
    return (k.abs()[:, :, :, None] * q.abs()[:, :, None, :]).sum(1)


def cct_chain(k, q, v, res, kd, qd, vd, idx=None):
    """The CCT algebra without its convolutions: out = res + gather(v, arg) * S + attn @ vd with (S, arg) = colmax(k^T q) and
    attn = colmax(kd^T qd).  idx: the two index tensors to replay (default: the reference's own first maxima)
    -> (out (B, C, n, n), [E, Ed], [arg, arg_d])"""
    B, C, n, _ = res.shape
    E, Ed = energy(k, q), energy(kd, qd)
    if idx is None:
        idx = [colmax(E.detach())[1], colmax(Ed.detach())[1]]
    S = select_rows(E, idx[0])
    T = gather_cols(v, idx[0])
    attn = select_rows(Ed, idx[1])
    out = res + mul_bcast_c(T, S.unsqueeze(1)).view(B, C, n, n) + bcast_matmul(attn.view(B, n, n), vd)
    return out, [E, Ed], idx
