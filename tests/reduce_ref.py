"""The block reduction of the measurement kernels (caesar_yolo_amd/csrc/cy_reduce.h) restated in numpy: entry q of a row on thread
q mod nt, sequential per thread over increasing q, a tree with offsets 32 .. 1 inside each wave of 64 (lane l takes lane l + o),
the waves added in order.  tree_sum is what tests/fit_ref.py and tests/aperture_ref.py add their sums with; the other
associations exist so that a test can show its inputs tell them apart; probe_rows is the reference of cy_debug_reduce."""
import numpy as np

LANES = 64
NONE32, NONE64, INT_MAX = 0xFFFFFFFF, (1 << 63) - 1, (1 << 31) - 1


def lane_sums(t, nt=256):
    """[k, n] -> [k, nt // 64, 64]: the sequential float64 sum every thread holds before the reduction."""
    k, n = t.shape
    rows = max(-(-n // nt), 1)
    x = np.zeros((k, rows * nt), np.float64)
    x[:, :n] = t
    x = x.reshape(k, rows, nt)
    acc = np.zeros((k, nt), np.float64)
    for r in range(rows):
        acc = acc + x[:, r]
    return acc.reshape(k, nt // LANES, LANES)


def wave_down(acc):
    """The kernel's step inside a wave: offsets 32 .. 1, the result in lane 0."""
    acc = acc.copy()
    for o in (32, 16, 8, 4, 2, 1):
        acc[:, :, :o] = acc[:, :, :o] + acc[:, :, o:2 * o]
    return acc[:, :, 0]


def wave_up(acc):
    """Not the kernel's: a butterfly that pairs neighbours first (offsets 1 .. 32)."""
    acc = acc.copy()
    for o in (1, 2, 4, 8, 16, 32):
        acc[:, :, ::2 * o] = acc[:, :, ::2 * o] + acc[:, :, o::2 * o]
    return acc[:, :, 0]


def waves_in_order(w):
    out = w[:, 0]
    for j in range(1, w.shape[1]):
        out = out + w[:, j]
    return out


def tree_sum(t, nt=256):
    """Sums of the rows of t [k, n] in the kernel's association."""
    return waves_in_order(wave_down(lane_sums(t, nt)))


def other_associations(t, nt=256):
    """name -> sums of the rows of t in an association that is NOT the kernel's (four waves)."""
    w = wave_down(lane_sums(t, nt))
    seq = np.zeros(t.shape[0], np.float64)
    for q in range(t.shape[1]):
        seq = seq + t[:, q]
    return {"waves reversed": waves_in_order(w[:, ::-1]),
            "waves pairwise": (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]),
            "up-sweep in the wave": waves_in_order(wave_up(lane_sums(t, nt))),
            "sequential": seq}


def probe_rows(val, key):
    """cy_debug_reduce's eight words per row (both finishing styles give these): val [rows, n] float64, key [rows, n] float32."""
    rows, n = val.shape
    out = np.zeros((rows, 8), np.uint64)
    out[:, 0] = tree_sum(val).view(np.uint64)
    out[:, 1] = n
    ok = (key != 0) & np.isfinite(key)
    for r in range(rows):
        idx = np.nonzero(ok[r])[0]
        if len(idx):
            first = int(idx[np.argmax(key[r, idx])])          # argmax returns the first of equal maxima; idx increases
            words = (int(key[r, first:first + 1].view(np.uint32)[0]), first, int(idx[0]), int(idx[-1]), first, int(idx[0]))
        else:
            words = (int(np.array([-np.inf], np.float32).view(np.uint32)[0]), NONE32, INT_MAX, (1 << 64) - 1, NONE64, (1 << 64) - 1)
        out[r, 2:] = np.array(words, np.uint64)
    return out
