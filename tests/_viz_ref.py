"""An independent numpy restatement of the byte rules behind the PNG output, written from the PNG specification (section 9,
filtering; section 12.8, the minimum-sum-of-absolute-differences heuristic) and the rules' own wording -- it imports nothing from ssdnerf_amd/viz.py.
Plain loops over rows and bytes: slow, and hard to get wrong in the same way as a vectorised or a wave-parallel version.

  quantise(pred, target=None)      (N, h, w, 3) operands, float32 or uint8 -> the scanlines (N, h, 3 W) uint8, target on the left
  filter_rows_ref(pred, target)    -> (N, h, 1 + 3 W) uint8: [type, filtered bytes] per row
  filter_types(rows)               -> the type bytes (N, h)
  unfilter(rows)                   -> (N, h, 3 W): the inverse, as a PNG reader computes it
  colour_map_ref(x, table, vmin, vmax)   float32 values -> (.., 3) uint8 through a 256-entry table, as matplotlib maps a float32 array
  plane_sheet_ref(code, flip_z)    (S, 3, C, h, w) -> (S, 3 h, C w): the reference's layout (triplane_decoder.py:186-191)
"""
import numpy as np


def _pred_bytes(x):
    if x.dtype == np.uint8:
        return x.copy()
    out = np.zeros(x.shape, np.uint8)
    flat, o = x.reshape(-1), out.reshape(-1)
    for i in range(flat.size):
        v = flat[i]
        if v != v:                                                       # NaN -> 0
            continue
        v = np.float32(min(max(v, np.float32(0)), np.float32(1))) * np.float32(255)        # one fp32 rounding
        o[i] = int(np.rint(v))                                           # ties to even
    return out


def _target_bytes(x):
    if x.dtype == np.uint8:
        return x.copy()
    out = np.zeros(x.shape, np.uint8)
    flat, o = x.reshape(-1), out.reshape(-1)
    for i in range(flat.size):
        v = flat[i]
        if v != v:
            continue
        v = np.float32(min(max(v, np.float32(0)), np.float32(1))) * np.float32(255)
        o[i] = int(v)                                                    # truncation
    return out


def quantise(pred, target=None):
    n, h, w, _ = pred.shape
    line = _pred_bytes(np.asarray(pred)).reshape(n, h, 3 * w)
    if target is not None:
        line = np.concatenate([_target_bytes(np.asarray(target)).reshape(n, h, 3 * w), line], axis=2)
    return line


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def _filter_line(cur, up):
    """the five filtered versions of one scanline (lists of ints), bpp = 3"""
    L = len(cur)
    out = [[0] * L for _ in range(5)]
    for i in range(L):
        x = cur[i]
        a = cur[i - 3] if i >= 3 else 0
        b = up[i]
        c = up[i - 3] if i >= 3 else 0
        out[0][i] = x
        out[1][i] = (x - a) % 256
        out[2][i] = (x - b) % 256
        out[3][i] = (x - (a + b) // 2) % 256
        out[4][i] = (x - _paeth(a, b, c)) % 256
    return out


def filter_lines_ref(lines):
    n, h, L = lines.shape
    rows = np.zeros((n, h, 1 + L), np.uint8)
    for k in range(n):
        for y in range(h):
            cur = lines[k, y].tolist()
            up = lines[k, y - 1].tolist() if y > 0 else [0] * L
            cands = _filter_line(cur, up)
            scores = [sum(min(r, 256 - r) for r in cand) for cand in cands]
            best = scores.index(min(scores))                             # the first minimum: a tie goes to the lowest filter number
            rows[k, y, 0] = best
            rows[k, y, 1:] = cands[best]
    return rows


def filter_rows_ref(pred, target=None):
    return filter_lines_ref(quantise(pred, target))


def filter_types(rows):
    return np.asarray(rows)[..., 0]


def unfilter(rows):
    rows = np.asarray(rows)
    n, h, L1 = rows.shape
    L = L1 - 1
    out = np.zeros((n, h, L), np.uint8)
    for k in range(n):
        prev = [0] * L
        for y in range(h):
            kind, src = int(rows[k, y, 0]), rows[k, y, 1:].tolist()
            cur = [0] * L
            for i in range(L):
                a = cur[i - 3] if i >= 3 else 0
                b = prev[i]
                c = prev[i - 3] if i >= 3 else 0
                pred = (0, a, b, (a + b) // 2, _paeth(a, b, c))[kind]
                cur[i] = (src[i] + pred) % 256
            out[k, y] = cur
            prev = cur
    return out


def colour_map_ref(x, table, vmin, vmax):
    x = np.asarray(x, np.float32)
    out = np.zeros(x.shape + (3,), np.uint8)
    span = np.float32(vmax) - np.float32(vmin)
    flat, o = x.reshape(-1), out.reshape(-1, 3)
    with np.errstate(all="ignore"):
        for i in range(flat.size):
            t = np.float32(np.float32(flat[i] - np.float32(vmin)) / span)
            if t != t:
                continue                                                 # NaN -> (0, 0, 0)
            if t < 0:
                o[i] = table[0]
            elif t >= 1:
                o[i] = table[255]
            else:
                o[i] = table[int(np.floor(np.float32(t * np.float32(256))))]
    return out


def plane_sheet_ref(code, flip_z):
    code = np.asarray(code)
    s, _, c, h, w = code.shape
    if not flip_z:
        code = code[..., ::-1, :]
    return code.transpose(0, 1, 3, 2, 4).reshape(s, 3 * h, c * w)


# ---------------------------------------------------------------------------------------------- the inputs both suites use
def crafted_image(h=10, w=67, seed=0):
    """(h, w, 3) uint8 whose rows favour different filters: noise; a copy of the row above; a ramp along the row; floor((a + b) / 2) of a noisy row
    above; a diagonal plane; constant rows"""
    g = np.random.default_rng(seed)
    img = np.zeros((h, w, 3), np.uint8)
    img[0] = g.integers(0, 256, (w, 3))
    if h > 1:
        img[1] = img[0]
    if h > 2:
        img[2] = (np.arange(w)[:, None] * 3 + np.arange(3)[None] * 40) % 256
    if h > 3:
        img[3] = g.integers(0, 256, (w, 3))
    if h > 4:                                                            # built left to right as the Average predictor of itself
        line, up = [0] * (3 * w), img[3].reshape(-1).tolist()
        for i in range(3 * w):
            line[i] = ((line[i - 3] if i >= 3 else 0) + up[i]) // 2
        img[4] = np.asarray(line, np.uint8).reshape(w, 3)
    for y in range(5, min(h, 8)):                                        # a plane: x + 2 y per channel, offset
        img[y] = ((np.arange(w)[:, None] * 2 + 5 * y + np.arange(3)[None] * 17) % 256)
    if h > 8:
        img[8:] = 131
    return img


def operand(u8, kind, seed=0, awkward=False):
    """``u8`` (.., 3) as an operand of the given kind: 'u8' as it is, 'f32' as k / 255 in float32.  ``awkward``: a few float32 elements are replaced by
    values outside [0, 1], ties at (k + 0.5) / 255, and NaN."""
    if kind == "u8":
        return np.ascontiguousarray(u8)
    x = (u8.astype(np.float32) / np.float32(255)).astype(np.float32)
    if awkward and x.size >= 12:
        flat = x.reshape(-1)
        g = np.random.default_rng(seed + 99)
        idx = g.choice(flat.size, size=min(flat.size, 40), replace=False)
        specials = np.float32([-0.5, 1.5, np.nan, 2.5 / 255, 3.5 / 255, 126.5 / 255, 127.5 / 255, 254.5 / 255, -0.0, 1.0, np.inf, -np.inf, 0.5 / 255])
        for j, i in enumerate(idx):
            flat[i] = specials[j % len(specials)]
    return x


SHAPES = [(10, 67, True), (10, 67, False), (1, 1, True), (1, 1, False), (3, 1, True), (1, 2, True), (1, 2, False)]        # (h, w, with target)
KINDS = [("f32", "f32"), ("f32", "u8"), ("u8", "f32"), ("u8", "u8")]                                                       # (pred, target)


def case(h, w, with_target, pred_kind, target_kind, n=2):
    """-> (pred, target or None) as numpy arrays (n, h, w, 3)"""
    pred = np.stack([operand(crafted_image(h, w, seed=10 + i), pred_kind, seed=i, awkward=True) for i in range(n)])
    target = None
    if with_target:
        target = np.stack([operand(crafted_image(h, w, seed=50 + i)[::-1 if i % 2 else 1], target_kind, seed=20 + i, awkward=True) for i in range(n)])
        target = np.ascontiguousarray(target)
    return np.ascontiguousarray(pred), target
