"""numpy float64 restatement of cy_atrous_step (include/caesar_yolo_hip.h): one level of the a trous B3-spline decomposition.

    a(x, y)     (double)in[y][x] when that value is finite, else 0.0
    fold(i, N)  0 when N == 1; otherwise p = 2 (N - 1), i = i mod p (non-negative), p - i when i >= N, else i
    h           (1/16, 1/4, 3/8, 1/4, 1/16)
    R(x, r)     h0 a(fold(x - 2s, MW), r), += h1 a(fold(x - s, MW), r), += h2 a(x, r), += h3 a(fold(x + s, MW), r), += h4 a(fold(x + 2s, MW), r)
    C(x, y)     the same five terms over R(x, fold(y + (k - 2) s, MH)), k = 0 .. 4
    smooth = (float)C;  detail = (float)(a - (double)(float)C)

Every product and every sum is one float64 operation, in this order, on both sides: the kernel's outputs equal these bit for bit.
atrous_step() works on whole folded index arrays; atrous_loops() is the same definition as plain nested loops over pixels with Python
integers for the indices (an independent statement of fold and of the order of the sums)."""
import numpy as np

H = (0.0625, 0.25, 0.375, 0.25, 0.0625)
STEP_MAX = 64


def fold(i, N):
    """Mirror without repeating the edge, for an integer array (or scalar) of any offsets."""
    i = np.asarray(i, np.int64)
    if N == 1:
        return np.zeros(i.shape, np.int64)
    p = 2 * (N - 1)
    m = np.mod(i, p)                                          # non-negative for a positive modulus
    return np.where(m >= N, p - m, m)


def values(img):
    """a: float64, non-finite values 0."""
    img = np.asarray(img, np.float32)
    return np.where(np.isfinite(img), img.astype(np.float64), 0.0)


def atrous_step(img, step):
    """-> (smooth float32 [MH, MW], detail float32 [MH, MW]) of the float32 map img."""
    a = values(img)
    MH, MW = a.shape
    s = int(step)
    assert 1 <= s <= STEP_MAX and a.ndim == 2
    x, y = np.arange(MW), np.arange(MH)
    R = H[0] * a[:, fold(x - 2 * s, MW)]
    for k in (1, 2, 3, 4):
        R = R + H[k] * a[:, fold(x + (k - 2) * s, MW)]
    C = H[0] * R[fold(y - 2 * s, MH), :]
    for k in (1, 2, 3, 4):
        C = C + H[k] * R[fold(y + (k - 2) * s, MH), :]
    with np.errstate(over="ignore"):
        smooth = C.astype(np.float32)
        detail = (a - smooth.astype(np.float64)).astype(np.float32)
    return smooth, detail


def fold_int(i, N):
    if N == 1:
        return 0
    p = 2 * (N - 1)
    i %= p                                                    # Python: non-negative
    return p - i if i >= N else i


def atrous_loops(img, step):
    """The definition pixel by pixel; for small maps."""
    img = np.asarray(img, np.float32)
    MH, MW = img.shape
    s = int(step)
    a = [[float(v) if np.isfinite(v) else 0.0 for v in row] for row in img]
    R = [[0.0] * MW for _ in range(MH)]
    for r in range(MH):
        for x in range(MW):
            t = H[0] * a[r][fold_int(x - 2 * s, MW)]
            t += H[1] * a[r][fold_int(x - s, MW)]
            t += H[2] * a[r][x]
            t += H[3] * a[r][fold_int(x + s, MW)]
            t += H[4] * a[r][fold_int(x + 2 * s, MW)]
            R[r][x] = t
    smooth, detail = np.zeros((MH, MW), np.float32), np.zeros((MH, MW), np.float32)
    with np.errstate(over="ignore"):
        for y in range(MH):
            for x in range(MW):
                t = H[0] * R[fold_int(y - 2 * s, MH)][x]
                t += H[1] * R[fold_int(y - s, MH)][x]
                t += H[2] * R[y][x]
                t += H[3] * R[fold_int(y + s, MH)][x]
                t += H[4] * R[fold_int(y + 2 * s, MH)][x]
                smooth[y, x] = np.float32(t)
                detail[y, x] = np.float32(a[y][x] - float(smooth[y, x]))
    return smooth, detail


def planes(img, nscales):
    """c_0 = img; for j = 1 .. nscales one step with 2^(j - 1) -> [(c_j, w_j)]."""
    out, c = [], np.asarray(img, np.float32)
    for j in range(1, nscales + 1):
        c, w = atrous_step(c, 1 << (j - 1))
        out.append((c, w))
    return out
