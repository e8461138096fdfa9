"""TEST INFRASTRUCTURE. Restatements of the streaming kernels that run between the products, the loss and the table passes of a
training step (tests/test_gpu_step_kernels.py holds the kernels against them; tests/test_step_kernels_reference.py holds THEM
against oracle/nvsm_oracle.py on small inputs, without a GPU).

Every formula takes a dtype: np.float64 is the reference, np.float32 the "plain float32 evaluation of the same formula" whose loss
against float64 scales the element-wise tolerances (the rule of tests/test_gpu_loss_shapes.py). Sums run over the window in window
order, over a row with numpy's own order. The scalars a kernel receives as floats (lr, lambda, eps, bc, 1 / dim) are inputs: the
float64 reference uses the float's value.

Two things are NOT float64: the ordered sums of the dT product's slabs and of the row-square parts are documented to the addition
(csrc/gather_gemm.hip) and emulated in float32, addition by addition; and the three bf16 pieces a float32 is cut into for the
projection products (csrc/gemm_split.hip split_pair) are emulated bit by bit. The byte offsets of the two plane layouts are written
here from the layout comments of gemm_split.hip and gemm_rsplit.hip; nothing in this file calls the product."""
import numpy as np

U32 = 2.0 ** -24
K_F32 = 4
SGD, ADAGRAD, ADAM = 0, 1, 2
BETA1, BETA2, OPT_EPS = np.float32(0.9), np.float32(0.999), np.float32(1e-6)


# ---- window passes -----------------------------------------------------------------------------------------------------------------
def window_sum(rows, idx, wts, dtype):
    """Σ_j wts[b, j] · rows[idx[b, j]] in window order, in dtype: [B] + rows.shape[1:]. Also Σ_j |term| (float64)."""
    rows = np.asarray(rows).astype(dtype)
    B, window = idx.shape
    acc = np.zeros((B,) + rows.shape[1:], dtype)
    mag = np.zeros((B,) + rows.shape[1:], np.float64)
    for j in range(window):
        term = rows[idx[:, j]]
        if wts is not None:
            w = np.asarray(wts)[:, j].astype(dtype)
            term = term * (w[:, None] if rows.ndim == 2 else w)
        acc = (acc + term).astype(dtype)
        mag += np.abs(term.astype(np.float64))
    return acc, mag


def gather_mean(table, idx, wts, dtype=np.float64):
    """phrase[b] = (Σ_j wts[b, j] · table[idx[b, j]]) / window (average_repr_kernel: the division is by the window even with weights).
    Returns (mean, Σ_j |term| / window)."""
    s, mag = window_sum(table, idx, wts, dtype)
    w = dtype(idx.shape[1])
    return (s / w).astype(dtype), mag / idx.shape[1]


def adam_u(m, v, idx, bc, eps, dtype=np.float64):
    """U[b] = bc · mean_j m[idx[b, j]] / (sqrt(mean_j v[idx[b, j]]) + eps)."""
    w = dtype(idx.shape[1])
    sm, _ = window_sum(m, idx, None, dtype)
    sv, _ = window_sum(v, idx, None, dtype)
    denom = (np.sqrt((sv / w).astype(dtype)) + dtype(eps)).astype(dtype)
    return (dtype(bc) * (sm / w).astype(dtype) / denom[:, None]).astype(dtype)


def adagrad_scale(acc, idx, eps, dtype=np.float64):
    """scale[b] = 1 / sqrt(mean_j acc[idx[b, j]] + eps)."""
    w = dtype(idx.shape[1])
    s, _ = window_sum(acc, idx, None, dtype)
    return (dtype(1) / np.sqrt(((s / w).astype(dtype) + dtype(eps)).astype(dtype))).astype(dtype)


# ---- batch-norm backward -------------------------------------------------------------------------------------------------------------
def bn_sums(dy, pre, mean, inv_std):
    """[2][dim] float64: Σ_rows dy and Σ_rows dy · xhat - what the loss kernel hands the backward."""
    dy, pre = np.asarray(dy, np.float64), np.asarray(pre, np.float64)
    xhat = (pre - np.asarray(mean, np.float64)) * np.asarray(inv_std, np.float64)
    return np.stack([dy.sum(axis=0), (dy * xhat).sum(axis=0)])


def bn_dx(dy, pre, mean, inv_std, sums, n_global, dtype=np.float64):
    """dx = inv_std · (dy − (dβ + xhat · dγ) / n_global), dβ and dγ the FLOAT casts of the float64 sums (cudnn per-activation
    backward). Returns (dx, dbeta, dgamma)."""
    db, dg = np.asarray(sums[0]).astype(np.float32).astype(dtype), np.asarray(sums[1]).astype(np.float32).astype(dtype)
    dy, pre, mean, inv_std = (np.asarray(a).astype(dtype) for a in (dy, pre, mean, inv_std))
    inv_n = dtype(np.float32(1.0 / n_global))
    xhat = ((pre - mean) * inv_std).astype(dtype)
    dx = (inv_std * (dy - ((db + (xhat * dg).astype(dtype)).astype(dtype) * inv_n).astype(dtype))).astype(dtype)
    return dx, db, dg


# ---- wave-per-row ops ----------------------------------------------------------------------------------------------------------------
def inv_dim_f32(dim):
    """1 / dim as launch_l2_rows_backward and launch_materialize_grad_entity_l2 form it: exp(−log(dim)) in double, then float."""
    return np.float32(np.exp(-np.log(np.float64(dim))))


def row_meansq(G, scale, dtype=np.float64):
    G = np.asarray(G).astype(dtype)
    return ((G * G).sum(axis=1, dtype=dtype) * dtype(scale)).astype(dtype)


def l2_forward(x, dtype=np.float64):
    """y = x / ‖x‖, norms = ‖x‖."""
    x = np.asarray(x).astype(dtype)
    n = np.sqrt((x * x).sum(axis=1, dtype=dtype)).astype(dtype)
    return (x / n[:, None]).astype(dtype), n


def l2_backward(g, x, norms, scale, dtype=np.float64):
    """gin = scale · (g · n² − x · (x · g)) / n³ (Normalizer::backward)."""
    g, x, n = (np.asarray(a).astype(dtype) for a in (g, x, norms))
    cr = (x * g).sum(axis=1, dtype=dtype).astype(dtype)
    n2 = (n * n).astype(dtype)
    n3 = (n2 * n).astype(dtype)
    return ((((g * n2[:, None]).astype(dtype) - (x * cr[:, None]).astype(dtype)) / n3[:, None]).astype(dtype) * dtype(scale)).astype(dtype)


def materialize(coef, proj, R, dtype=np.float64):
    """grad_entity[j] = coef[j] · proj[j // R]."""
    coef, proj = np.asarray(coef).astype(dtype), np.asarray(proj).astype(dtype)
    src = np.arange(coef.size) // R
    return (proj[src] * coef[:, None]).astype(dtype)


def materialize_l2(coef, proj, E, ids, R, dtype=np.float64):
    """g_j = coef[j] · proj[j // R] sent back through the normaliser with the raw row E[ids[j]] as its cached input, the norm
    recomputed from the row."""
    g = materialize(coef, proj, R, dtype)
    e = np.asarray(E).astype(dtype)[ids]
    _, n = l2_forward(e, dtype)
    return l2_backward(g, e, n, 1.0, dtype)


# ---- the two ordered float32 sums ----------------------------------------------------------------------------------------------------
def splitk_reduce_f32(parts):
    """launch_splitk_reduce's float4 kernel, addition by addition: group j (of sixteen) starts at 0 and adds slabs j, j + 16, j + 32,
    ... in that order; then the sixteen group sums are added in group order, starting from group 0's."""
    parts = np.asarray(parts, np.float32)
    groups = np.zeros((16,) + parts.shape[1:], np.float32)
    for z in range(parts.shape[0]):
        groups[z % 16] = groups[z % 16] + parts[z]
    t = groups[0].copy()
    for k in range(1, 16):
        t = t + groups[k]
    return t


def splitk_reduce_scalar_f32(parts):
    """... and its scalar kernel (n or the stride no multiple of 4): 0, then the slabs in slab order."""
    parts = np.asarray(parts, np.float32)
    s = np.zeros(parts.shape[1:], np.float32)
    for z in range(parts.shape[0]):
        s = s + parts[z]
    return s


def sum_parts_f32(parts):
    """launch_sum_parts: part 0, then the others added in part order."""
    parts = np.asarray(parts, np.float32)
    s = parts[0].copy()
    for p in range(1, parts.shape[0]):
        s = s + parts[p]
    return s


# ---- the dense optimiser of (T, b) -----------------------------------------------------------------------------------------------------
def adam_bc(t, dtype=np.float64):
    b1, b2 = np.float64(BETA1), np.float64(BETA2)
    return dtype(np.sqrt(1.0 - b2 ** np.float64(t)) / (1.0 - b1 ** np.float64(t)))


def transform_update(method, T, b, gT, gb, s0T, s0b, s1T, s1b, lr, lam, t, dtype=np.float64):
    """One update of the projection (TransformUpdater::update with the reference's quirks): λ decays T only - through the decay
    factor 1 − λ · lr for SGD and Adagrad, folded into the gradient for Adam -, and the Adam moments of the bias are scaled by 1
    where those of T are scaled by β. Returns a dict of the new T, b, gT, gb (the applied direction; SGD leaves the gradient) and
    state. lr and lam are the floats the kernel receives."""
    f = lambda a: None if a is None else np.asarray(a).astype(dtype)
    T, b, gT, gb, s0T, s0b, s1T, s1b = (f(a) for a in (T, b, gT, gb, s0T, s0b, s1T, s1b))
    lr, lam, eps = dtype(np.float32(lr)), dtype(np.float32(lam)), dtype(OPT_EPS)
    dec = dtype(1.0 - np.float64(np.float32(lam)) * np.float64(np.float32(lr)))
    out = {}
    if method == SGD:
        out.update(T=T * dec + gT * lr, b=b * dtype(1) + gb * lr, gT=gT, gb=gb)
    elif method == ADAGRAD:
        aT, ab = s0T + gT * gT, s0b + gb * gb
        dT, db = gT / np.sqrt(aT + eps), gb / np.sqrt(ab + eps)
        out.update(T=T * dec + dT * lr, b=b + db * lr, gT=dT, gb=db, s0T=aT, s0b=ab)
    else:
        one_m_b1, one_m_b2 = dtype(1.0 - np.float64(BETA1)), dtype(1.0 - np.float64(BETA2))
        s_m, s_v = dtype(1.0 - np.float64(one_m_b1)), dtype(1.0 - np.float64(one_m_b2))
        bc = adam_bc(t, dtype)
        g = (gT + (-lam) * T).astype(dtype)
        mT, vT = s0T * s_m + g * one_m_b1, s1T * s_v + (g * g) * one_m_b2
        mb, vb = s0b * dtype(1) + gb * one_m_b1, s1b * dtype(1) + (gb * gb) * one_m_b2
        dT, db = (mT * bc) / (np.sqrt(vT) + eps), (mb * bc) / (np.sqrt(vb) + eps)
        out.update(T=T + dT * lr, b=b + db * lr, gT=dT, gb=db, s0T=mT, s0b=mb, s1T=vT, s1b=vb)
    return {k: np.asarray(v).astype(dtype) for k, v in out.items()}


# ---- bf16 pieces and the plane layouts -------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), returned as its 16 bits (uint16). Finite inputs."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return r.astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """h = bf16(x), m = bf16(x − h), l = bf16(x − h − m), the differences in float32 (exact): three uint16 arrays."""
    x = np.ascontiguousarray(x, np.float32)
    h = bf16_round(x)
    r = (x - bf16_value(h)).astype(np.float32)
    m = bf16_round(r)
    s = (r - bf16_value(m)).astype(np.float32)
    return h, m, bf16_round(s)


def plane_geometry(kind, N, K):
    """(bytes of one plane, bytes of the buffer) of an operand B with K rows (the summed dimension) and N columns.
    kind 1, gemm_split.hip: planes[3][ceil(K / 32)][np][32] bf16, np = N padded to 16 columns, + 2 KB behind the last plane.
    kind 2, gemm_rsplit.hip: planes[3][KSP][NT][64][8] bf16, KSP = k steps of 16 padded to an even number, NT = 32-column tiles."""
    if kind == 1:
        stride = ((K + 31) // 32) * (16 * ((N + 15) // 16)) * 64
        return stride, 3 * stride + 2048
    ks = (K + 15) // 16
    stride = (ks + (ks & 1)) * ((N + 31) // 32) * 1024
    return stride, 3 * stride


def plane_offset(kind, N, K, k, n):
    """Byte offset of element (k, n) inside one plane (k, n may be arrays).
    kind 1: [k // 32][n][k % 32], two bytes each.
    kind 2: element j of lane l of (ks, tile) is B(k = 16 ks + 8 (l >> 5) + j, n = 32 tile + (l & 31)): [k // 16][n // 32][lane][k % 8]
    with lane = n % 32 + 32 · ((k % 16) // 8)."""
    k, n = np.asarray(k, np.int64), np.asarray(n, np.int64)
    if kind == 1:
        npad = 16 * ((N + 15) // 16)
        return ((k // 32) * npad + n) * 64 + (k % 32) * 2
    nt = (N + 31) // 32
    lane = n % 32 + 32 * ((k % 16) // 8)
    return (((k // 16) * nt + n // 32) * 64 + lane) * 16 + (k % 8) * 2


def decode_planes(kind, N, K, buf):
    """The three [K][N] uint16 piece arrays a plane buffer holds."""
    stride, _ = plane_geometry(kind, N, K)
    k, n = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    off = plane_offset(kind, N, K, k, n)
    buf = np.asarray(buf, np.uint8)
    return [buf[off + p * stride].astype(np.uint16) | (buf[off + p * stride + 1].astype(np.uint16) << 8) for p in range(3)]


def encode_planes(kind, N, K, B):
    """The 3 · plane_stride bytes of the planes of B [K][N] float32, zero outside the matrix."""
    stride, _ = plane_geometry(kind, N, K)
    out = np.zeros(3 * stride, np.uint8)
    k, n = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    off = plane_offset(kind, N, K, k, n)
    for p, piece in enumerate(split3(B)):
        out[off + p * stride] = (piece & 0xFF).astype(np.uint8)
        out[off + p * stride + 1] = (piece >> 8).astype(np.uint8)
    return out


# ---- tolerances ------------------------------------------------------------------------------------------------------------------------
def elementwise_tol(ref64, ref32):
    """K_F32 times what the plain float32 evaluation loses against float64 over the tensor, plus 1e-6 of the tensor's largest
    magnitude (tests/test_gpu_loss_shapes.py, tests/test_gpu_magnitudes.py)."""
    ref64 = np.asarray(ref64, np.float64)
    return K_F32 * np.abs(np.asarray(ref32, np.float64) - ref64).max() + 1e-6 * np.abs(ref64).max()


def wave_sum_additions(dim):
    """float32 additions on the longest chain of a wave's row sum, plus 2: a lane's ceil(dim / 64) elements, six shuffle steps."""
    return (dim + 63) // 64 + 6 + 2
