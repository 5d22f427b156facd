"""numpy restatement of the per-region overlap (csrc/region_overlap.hip, metrics.ProHistogram) for the tests: a labeller with the
device's canonical labels, the integer region weights, the state as exact integers, and AUPRO in float64 straight from its
definition.  Also the fixture masks that defeat a labeller with a too-small iteration bound."""
import numpy as np

import pixel_metrics_ref as hist_ref

WEIGHT_BITS = 44


def positive(masks, fmt):
    """'u8': anomalous iff >= 128; 'f32': iff > 0.5."""
    return hist_ref.positive(masks, fmt)


def label(mask, connectivity=8):
    """mask: bool [h, w].  -> (labels int32 [h, w], sizes uint32 [h, w]): labels 0 = normal, otherwise 1 + (the smallest y * w + x of
    the pixel's region); sizes = the region's pixel count at that smallest pixel, 0 elsewhere.  Union-find in raster order, the
    larger root always hung below the smaller, so a root is its region's smallest index."""
    mask = np.asarray(mask, dtype=bool)
    h, w = mask.shape
    parent = list(range(h * w))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    if connectivity == 8:
        steps = ((0, -1), (-1, -1), (-1, 0), (-1, 1))
    elif connectivity == 4:
        steps = ((0, -1), (-1, 0))
    else:
        raise ValueError(connectivity)
    flat = mask.reshape(-1)
    for i in np.flatnonzero(flat).tolist():
        y, x = divmod(i, w)
        for dy, dx in steps:
            yy, xx = y + dy, x + dx
            if yy >= 0 and 0 <= xx < w and flat[yy * w + xx]:
                a, b = find(i), find(yy * w + xx)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    labels = np.zeros(h * w, np.int32)
    sizes = np.zeros(h * w, np.uint32)
    for i in np.flatnonzero(flat).tolist():
        r = find(i)
        labels[i] = r + 1
        sizes[r] += 1
    return labels.reshape(h, w), sizes.reshape(h, w)


def kernel_links(mask, connectivity=8):
    """The links the merge kernel makes (csrc/region_overlap.hip), as (pixel, neighbour) index pairs: under 8-connectivity one or
    two per pixel instead of four - with the pixel above set only that one; otherwise left, or else above-left, and above-right."""
    mask = np.asarray(mask, dtype=bool)
    h, w = mask.shape
    out = []
    for i in np.flatnonzero(mask.reshape(-1)).tolist():
        y, x = divmod(i, w)
        left = x > 0 and mask[y, x - 1]
        up = y > 0 and mask[y - 1, x]
        if connectivity == 4:
            out += [(i, i - 1)] * bool(left) + [(i, i - w)] * bool(up)
        elif up:
            out.append((i, i - w))
        else:
            upleft = y > 0 and x > 0 and mask[y - 1, x - 1]
            upright = y > 0 and x + 1 < w and mask[y - 1, x + 1]
            if left:
                out.append((i, i - 1))
            elif upleft:
                out.append((i, i - w - 1))
            if upright:
                out.append((i, i - w + 1))
    return out


def label_batch(masks, connectivity=8):
    """masks: bool [n, h, w], every image on its own.  -> (labels int32 [n, h, w], sizes uint32 [n, h, w])."""
    out = [label(m, connectivity) for m in masks]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def weight(size):
    """W(r) = (2^44 + |r| / 2) / |r| in integer division."""
    size = int(size)
    return ((1 << WEIGHT_BITS) + size // 2) // size


def region_sizes(labels):
    """labels int32 [n, h, w] -> the size of every pixel's region, int64 [n, h, w] (0 at normal pixels)."""
    labels = np.asarray(labels)
    n = labels.shape[0]
    flat = labels.reshape(n, -1)
    out = np.zeros(flat.shape, np.int64)
    for i in range(n):
        cnt = np.bincount(flat[i][flat[i] > 0] - 1, minlength=flat.shape[1])
        out[i] = np.where(flat[i] > 0, cnt[np.maximum(flat[i] - 1, 0)], 0)
    return out.reshape(labels.shape)


def ref_state(values, pos, labels, m):
    """values float32 [n, h, w], pos bool [n, h, w], labels int32 [n, h, w] (of pos).  -> dict of exact integers: 'wpos' (uint64
    [nbins]: integer sums, checked against a Python-integer total so that none can have wrapped), 'pos', 'neg' (int64 [nbins]),
    'regions', 'max_region', 'rejected' (int64 [2]: normal, anomalous)."""
    values = np.asarray(values, np.float32)
    pos = np.asarray(pos, dtype=bool)
    labels = np.asarray(labels)
    assert values.shape == pos.shape == labels.shape and np.array_equal(labels > 0, pos)
    counts, rejected = hist_ref.ref_counts(values, pos, m)
    key, ok = hist_ref.keys_of(values, m)
    sizes = region_sizes(labels).reshape(-1)
    binned = np.flatnonzero(ok & pos.reshape(-1))
    by_size = {int(s): weight(s) for s in np.unique(sizes[binned]).tolist()}
    weights = np.array([by_size[int(s)] for s in sizes[binned].tolist()], np.uint64)
    assert sum(by_size[int(s)] for s in sizes[binned].tolist()) < 1 << 64
    wpos = np.zeros(hist_ref.nbins(m), np.uint64)
    np.add.at(wpos, key[binned], weights)
    n = labels.shape[0]
    flat = labels.reshape(n, -1)
    roots = flat == (np.arange(flat.shape[1], dtype=np.int64) + 1)[None]
    return {"wpos": wpos, "pos": counts[1], "neg": counts[0], "regions": int(roots.sum()),
            "max_region": int(sizes.max()) if sizes.size else 0, "rejected": rejected}


def wpos_bits(wpos):
    """The uint64 sums as the int64 view the device's counters are read through."""
    return np.asarray(wpos, dtype=np.uint64).view(np.int64)


def state_words(st):
    """The reference state as the int64 words behind the blob's header: wpos, pos, neg, regions, max_region, rejected[2], flags 0."""
    tail = np.array([st["regions"], st["max_region"], st["rejected"][0], st["rejected"][1], 0], np.int64)
    return np.concatenate([wpos_bits(st["wpos"]), st["pos"].astype(np.int64), st["neg"].astype(np.int64), tail])


def aupro_oracle(scores, labels, pos, fpr_limit):
    """AUPRO in float64 from the definition: one threshold per distinct score, FPR(t) = the share of normal pixels with score >= t,
    PRO(t) = the mean over regions of the share of the region's pixels with score >= t; the points after (0, 0) joined by straight
    lines, integrated up to fpr_limit with one interpolation on the segment it cuts, divided by fpr_limit."""
    scores = np.asarray(scores, np.float64)
    pos = np.asarray(pos, dtype=bool)
    labels = np.asarray(labels)
    assert scores.shape == pos.shape == labels.shape and np.all(np.isfinite(scores)) and np.all(scores >= 0)
    sizes = region_sizes(labels)
    n = labels.shape[0]
    regions = int((labels.reshape(n, -1) == (np.arange(labels[0].size) + 1)[None]).sum())
    s, p, sz = scores.reshape(-1), pos.reshape(-1), sizes.reshape(-1)
    thresholds = np.unique(s)[::-1]
    n_neg = int((~p).sum())
    fpr, pro = [0.0], [0.0]
    neg_scores = np.sort(s[~p])
    order = np.argsort(-s[p], kind="stable")
    pos_scores = s[p][order]
    share = np.cumsum((1.0 / sz[p][order].astype(np.float64)))
    for t in thresholds:
        fpr.append((n_neg - np.searchsorted(neg_scores, t, side="left")) / n_neg)
        k = np.searchsorted(-pos_scores, -t, side="right")              # anomalous pixels with score >= t
        pro.append((share[k - 1] if k else 0.0) / regions)
    fpr, pro = np.array(fpr), np.array(pro)
    area = 0.0
    for k in range(1, len(fpr)):
        if fpr[k] <= fpr_limit:
            area += (fpr[k] - fpr[k - 1]) * (pro[k] + pro[k - 1]) * 0.5
        else:
            cut = pro[k - 1] + (pro[k] - pro[k - 1]) * (fpr_limit - fpr[k - 1]) / (fpr[k] - fpr[k - 1])
            area += (fpr_limit - fpr[k - 1]) * (pro[k - 1] + cut) * 0.5
            break
    return area / fpr_limit


# ------------------------------------------------------------------------------------------ masks
def blobs(rng, n, h, w, count=6, radius=6):
    """n masks of a few random discs and bars each (some overlapping, some touching the border)."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((n, h, w), bool)
    for i in range(n):
        for _ in range(count):
            cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(1, radius + 1)
            if rng.random() < 0.5:
                out[i] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
            else:
                out[i] |= (abs(yy - cy) <= 0) & (abs(xx - cx) <= 2 * r)
    return out


def u_shape(h, w):
    """Two arms along the left and right edges that join only in the last row."""
    m = np.zeros((h, w), bool)
    m[:, 0] = m[:, -1] = m[-1, :] = True
    return m


def serpentine(h, w):
    """Every second row set, joined alternately at the right and the left end: one region, a path of ~h * w / 2 pixels."""
    m = np.zeros((h, w), bool)
    m[::2] = True
    for k, y in enumerate(range(1, h, 2)):
        m[y, -1 if k % 2 == 0 else 0] = True
    return m


def spiral(n):
    """A rectangular spiral of one-pixel walls and one-pixel gaps on n x n: one 4-connected path from the corner to the centre."""
    m = np.zeros((n, n), bool)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = True
    run = n - 1
    turns = 0
    while run > 0:
        for _ in range(run):
            y, x = y + dy, x + dx
            m[y, x] = True
        dy, dx = dx, -dy
        turns += 1
        if turns == 3 or (turns > 3 and (turns - 3) % 2 == 0):
            run -= 2
    return m
