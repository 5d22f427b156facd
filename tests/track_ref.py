"""numpy restatement of the event tracker (csrc/map_track.hip, metrics.EventTracker) for the tests, frame by frame and from the
specification alone: the slot plane, the open table, merges, the closing order, the filters, truncation,
lost events, the counts and the causal frame counts.  Built on the 2-D labeller of tests/pro_ref.py and the predicate and order key
of tests/regions_ref.py; `convert` turns tracker records into the 16-word records of tests/events_ref.py."""
import numpy as np

import events_ref
import pro_ref
import regions_ref

WORDS = 20
ROOT_PIXEL, T0, T1, HANDLE, X0, Y0, X1, Y1, PEAK, PEAK_PIXEL, PEAK_FRAME, RESERVED, VOLUME, SUM_X, SUM_Y, SUM_T = (
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 18)
HEADER_WORDS = 16
NO_RECORD = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def _u64(rec, col):
    return int(rec[col]) | (int(rec[col + 1]) << 32)


def _put64(rec, col, value):
    value &= MASK64
    rec[col], rec[col + 1] = value & 0xFFFFFFFF, value >> 32


def pack(e):
    """An open or closed event (dict of Python integers) -> its 20 words."""
    rec = np.zeros(WORDS, np.uint32)
    rec[ROOT_PIXEL], rec[T0], rec[T1], rec[HANDLE] = e["root_pixel"], e["t0"], e["t1"], e["handle"]
    rec[X0], rec[Y0], rec[X1], rec[Y1] = e["box"]
    rec[PEAK], rec[PEAK_PIXEL], rec[PEAK_FRAME] = e["peak_bits"], e["peak_pixel"], e["peak_frame"]
    for col, name in ((VOLUME, "volume"), (SUM_X, "sum_x"), (SUM_Y, "sum_y"), (SUM_T, "sum_t")):
        _put64(rec, col, e[name])
    return rec


def convert(records, h, w):
    """Tracker records [k, 20] in use -> the records of events_ref [k, 16], sorted by root: root = t0 * h * w + root_pixel, peak
    index = peak_frame * h * w + peak_pixel.  The volume must fit 32 bits."""
    records = np.asarray(records, np.uint32).reshape(-1, WORDS)
    out = np.zeros((len(records), events_ref.WORDS), np.uint32)
    for k, r in enumerate(records):
        volume = _u64(r, VOLUME)
        assert 0 < volume < 2 ** 32 and r[RESERVED] == 0
        out[k, events_ref.ROOT] = int(r[T0]) * h * w + int(r[ROOT_PIXEL])
        out[k, events_ref.VOLUME] = volume
        out[k, events_ref.T0], out[k, events_ref.T1] = r[T0], r[T1]
        out[k, events_ref.X0:events_ref.Y1 + 1] = r[X0:Y1 + 1]
        out[k, events_ref.PEAK] = r[PEAK]
        out[k, events_ref.PEAK_INDEX] = int(r[PEAK_FRAME]) * h * w + int(r[PEAK_PIXEL])
        out[k, events_ref.SUM_X:events_ref.SUM_X + 6] = r[SUM_X:SUM_X + 6]
    return out[np.argsort(out[:, events_ref.ROOT], kind="stable")]


class Tracker:
    """One stream.  `table`: the open events with a record, in slot order; `plane`: uint32 [h * w], 0, slot + 1 or NO_RECORD."""

    def __init__(self, h, w, threshold, connectivity=8, temporal=9, min_duration=1, min_volume=1, max_open=1024, max_closed=64):
        assert connectivity in (4, 8) and temporal in (1, 9) and (temporal == 1 or connectivity == 8)
        assert min_duration >= 1 and min_volume >= 1 and 1 <= max_open <= 65536 and 1 <= max_closed <= 65536
        self.h, self.w, self.threshold, self.connectivity, self.temporal = h, w, np.float32(threshold), connectivity, temporal
        self.min_duration, self.min_volume, self.max_open, self.max_closed = min_duration, min_volume, max_open, max_closed
        self.reset()

    def reset(self):
        self.frames, self.lost_total, self.table = 0, 0, []
        self.plane = np.zeros(self.h * self.w, np.uint32)

    def _passes(self, e):
        return e["t1"] - e["t0"] + 1 >= self.min_duration and e["volume"] >= self.min_volume

    def _frame(self, frame, out):
        h, w, f = self.h, self.w, self.frames
        frame = np.ascontiguousarray(frame, np.float32).reshape(h, w)
        fg = regions_ref.foreground(frame, self.threshold)
        labels, _ = pro_ref.label(fg, self.connectivity)
        flat = labels.reshape(-1).astype(np.int64)
        keys = regions_ref.order_key(frame.reshape(-1))
        bits = frame.reshape(-1).view(np.uint32)
        # which open events does every region of the new frame link to?  (pixel behind it; under temporal 9 its 3 x 3)
        before = np.zeros((h + 2, w + 2), np.int64)
        before[1:-1, 1:-1] = self.plane.reshape(h, w)
        shifts = [(0, 0)] if self.temporal == 1 else [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        parent = {}

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        roots = np.unique(flat[flat != 0] - 1).tolist()
        for r in roots:
            parent[("r", r)] = ("r", r)
        for dy, dx in shifts:
            behind = before[1 + dy:1 + dy + h, 1 + dx:1 + dx + w].reshape(-1)
            hit = (flat != 0) & (behind >= 1) & (behind <= self.max_open)      # a lost event's pixels are background for the links
            for r, s in set(zip((flat[hit] - 1).tolist(), (behind[hit] - 1).tolist())):
                parent.setdefault(("s", s), ("s", s))
                a, b = find(("r", r)), find(("s", s))
                if a != b:
                    parent[a] = b
        groups = {}
        for r in roots:
            groups.setdefault(find(("r", r)), {"regions": [], "old": []})["regions"].append(r)
        closing = []
        for s, e in enumerate(self.table):
            if ("s", s) in parent:
                groups[find(("s", s))]["old"].append(e)
            else:
                closing.append(e)
        # the events without a link closed: slot order, filters, truncation
        for e in closing:
            self._close(e, out)
        ordered = sorted(groups.values(), key=lambda g: min(g["regions"]))
        table, plane, alarm = [], np.zeros(h * w, np.uint32), 0
        for rank, g in enumerate(ordered):
            handle = min(g["regions"])
            pix = np.flatnonzero(np.isin(flat, np.asarray(g["regions"]) + 1))
            if rank >= self.max_open:                                           # no record: lost, once; its old records go with it
                plane[pix] = NO_RECORD
                out["lost"] += 1
                self.lost_total += 1
                continue
            y, x = pix // w, pix % w
            cands = [(int(keys[i]), f, int(i)) for i in pix] + [(int(regions_ref.order_key(np.array([o["peak_bits"]], np.uint32).view(np.float32))[0]),
                                                                  o["peak_frame"], o["peak_pixel"]) for o in g["old"]]
            key, pf, pp = min(cands, key=lambda c: (-c[0], c[1], c[2]))
            peak_bits = int(bits[pp]) if pf == f else next(o["peak_bits"] for o in g["old"] if (o["peak_frame"], o["peak_pixel"]) == (pf, pp))
            t0, root_pixel = min([(f, handle)] + [(o["t0"], o["root_pixel"]) for o in g["old"]])
            e = {"root_pixel": root_pixel, "t0": t0, "t1": f, "handle": handle,
                 "box": (min([int(x.min())] + [o["box"][0] for o in g["old"]]), min([int(y.min())] + [o["box"][1] for o in g["old"]]),
                         max([int(x.max())] + [o["box"][2] for o in g["old"]]), max([int(y.max())] + [o["box"][3] for o in g["old"]])),
                 "peak_bits": peak_bits, "peak_pixel": pp, "peak_frame": pf,
                 "volume": len(pix) + sum(o["volume"] for o in g["old"]),
                 "sum_x": int(x.sum()) + sum(o["sum_x"] for o in g["old"]), "sum_y": int(y.sum()) + sum(o["sum_y"] for o in g["old"]),
                 "sum_t": (f * len(pix) + sum(o["sum_t"] for o in g["old"])) & MASK64}
            table.append(e)
            plane[pix] = rank + 1
            if self._passes(e):
                alarm += len(pix)
        self.table, self.plane = table, plane
        self.frames += 1
        nan = int(np.isnan(frame).sum())
        out["fg"] += int(fg.sum())
        out["nan"] += nan
        out["frame_counts"].append([int(fg.sum()), alarm, nan])

    def _close(self, e, out):
        if self._passes(e):
            if out["kept"] < self.max_closed:
                out["closed"][out["kept"]] = pack(e)
            out["kept"] += 1
        else:
            out["dropped"] += 1

    def _result(self, out):
        counts = np.array([out["kept"], out["dropped"], out["fg"], out["nan"], len(self.table), out["lost"]], np.uint32)
        return out["closed"], counts, np.asarray(out["frame_counts"], np.uint32).reshape(-1, 3)

    def _fresh(self):
        return {"closed": np.zeros((self.max_closed, WORDS), np.uint32), "kept": 0, "dropped": 0, "fg": 0, "nan": 0, "lost": 0, "frame_counts": []}

    def update(self, maps):
        """maps float32 [t, h, w], t >= 1 -> (closed uint32 [max_closed, 20], counts uint32 [6], frame_counts uint32 [t, 3])."""
        maps = np.asarray(maps, np.float32).reshape(-1, self.h, self.w)
        assert len(maps) >= 1
        out = self._fresh()
        for frame in maps:
            self._frame(frame, out)
        return self._result(out)

    def flush(self):
        """Every open event closes, in slot order, as if an empty frame had arrived; the counter stands."""
        out = self._fresh()
        for e in self.table:
            self._close(e, out)
        self.table, self.plane = [], np.zeros(self.h * self.w, np.uint32)
        closed, counts, _ = self._result(out)
        return closed, counts

    def open_table(self):
        """uint32 [max_open, 20]: the open records in slot order, zeros behind."""
        t = np.zeros((self.max_open, WORDS), np.uint32)
        for s, e in enumerate(self.table):
            t[s] = pack(e)
        return t


def run(maps, splits, **kw):
    """One stream's maps [t, h, w] fed in calls of the given lengths (they sum to t), then flushed -> dict: 'closed' (the records in
    use of every call and of the flush, concatenated, [k, 20]), 'counts' [calls + 1, 6], 'frame_counts' [t, 3], 'table'
    [max_open, 20] and 'plane' [h * w] before the flush, 'lost' (in total), 'truncated' (any call)."""
    maps = np.asarray(maps, np.float32)
    t, h, w = maps.shape
    assert sum(splits) == t
    tr = Tracker(h, w, **kw)
    closed, counts, frames, at, truncated = [], [], [], 0, False
    for n in splits:
        c, k, fc = tr.update(maps[at:at + n])
        at += n
        closed.append(c[:min(int(k[0]), tr.max_closed)])
        truncated |= int(k[0]) > tr.max_closed
        counts.append(k)
        frames.append(fc)
    table, plane = tr.open_table(), tr.plane.copy()
    c, k = tr.flush()
    closed.append(c[:min(int(k[0]), tr.max_closed)])
    truncated |= int(k[0]) > tr.max_closed
    counts.append(k)
    return {"closed": np.concatenate(closed), "counts": np.stack(counts), "frame_counts": np.concatenate(frames), "table": table, "plane": plane,
            "lost": tr.lost_total, "truncated": truncated, "frames": tr.frames}
