"""Host model of an upload's policy (csrc/upload_plan.cpp), written from the loops gs_mesh_upload_from, mesh_commit_segment,
mesh_range_slotted, gs_mesh_bounds and mesh_staging_layout had before the policy was one file - over a bitmap of the splats that
own storage slots, not over ranges:

  * the ranges are the bitmap's runs (runs that touch are one run);
  * an upload of [from, end) is cut where the bitmap changes; a segment is fresh iff none of its splats is slotted and non-fresh
    iff all of them are;
  * a fresh segment (every segment of a mesh that keeps upload order) has the boxes of its own span redone, a non-fresh one those
    of the run that holds it - before the upload's own merge; b0 = lo // 256, b1 = ceil(hi / 256).

The bitmap has one cell per stretch between two neighbouring points that matter (the ends of every range and span involved), so
that spans up to 2^28 cost nothing; every cell is slotted as a whole or not at all.  Python integers: no sum wraps."""

BLOCK = 256
MAX_SPLATS = 1 << 28


class Bitmap:
    def __init__(self, ranges, *spans):
        """ranges: [begin, end) pairs, added in any order, overlapping or not; spans: further (begin, end) whose ends are cell borders."""
        pts = {0}
        for b, e in list(ranges) + list(spans):
            assert 0 <= b <= e
            pts.update((b, e))
        self.pts = sorted(pts)
        self.bit = [False] * (len(self.pts) - 1)
        for b, e in ranges:
            self.set(b, e)

    def cells(self, b, e):
        return [k for k in range(len(self.bit)) if b <= self.pts[k] and self.pts[k + 1] <= e]

    def set(self, b, e):
        for k in self.cells(b, e):
            self.bit[k] = True

    def runs(self):
        out = []
        for k, on in enumerate(self.bit):
            if not on:
                continue
            if out and out[-1][1] == self.pts[k]:
                out[-1][1] = self.pts[k + 1]
            else:
                out.append([self.pts[k], self.pts[k + 1]])
        return [tuple(r) for r in out]

    def cut(self, b, e):
        """[b, e) as consecutive (begin, end, fresh): a new segment wherever the bit changes."""
        out = []
        for k in self.cells(b, e):
            if out and out[-1][2] == (not self.bit[k]):
                out[-1][1] = self.pts[k + 1]
            else:
                out.append([self.pts[k], self.pts[k + 1], not self.bit[k]])
        return [tuple(s) for s in out]

    def holding(self, start, count):
        """The run that contains [start, start + count) whole, or None."""
        for b, e in self.runs():
            if b <= start and start + count <= e:
                return (b, e)
        return None


def plan_upload(ranges, start, count, reorder):
    """[(begin, end, fresh, b0, b1)] of an upload of [start, start + count) into a mesh whose slotted splats are `ranges`."""
    end = start + count
    assert end <= MAX_SPLATS
    bm = Bitmap(ranges, (start, end))
    out = []
    for b, e, fresh in bm.cut(start, end):
        assert all(not bm.bit[k] for k in bm.cells(b, e)) if fresh else all(bm.bit[k] for k in bm.cells(b, e))
        fresh = fresh or not reorder
        lo, hi = (b, e) if fresh else bm.holding(b, e - b)
        out.append((b, e, int(fresh), lo // BLOCK, -(-hi // BLOCK)))
    return out


def ranges_after(ranges, start, count):
    bm = Bitmap(ranges, (start, start + count))
    bm.set(start, start + count)
    return bm.runs()


def upload_layout(count, cov_half, mesh_sh_u8, sh_degree, source_stages_sh_u8):
    """mesh_staging_layout: centres | covariances | SH | rgba, every plane on a multiple of 256 bytes, and the room it asks for."""
    up = lambda v: (v + 255) // 256 * 256
    ncoef = 0 if sh_degree == 0 or (mesh_sh_u8 and not source_stages_sh_u8) else (9 if sh_degree == 1 else 24)
    sh_u8 = bool(mesh_sh_u8 and ncoef)
    b_sh = count * ncoef * (1 if sh_u8 else 2)
    off_cov = up(count * 12)
    off_sh = up(off_cov + count * (12 if cov_half else 24))
    return {"ncoef": ncoef, "sh_u8": int(sh_u8), "off_cov": off_cov, "off_sh": off_sh, "off_rgba": up(off_sh + b_sh),
            "bytes": off_sh + b_sh + 512 + count * 4}


def upload_plan(i):
    """Everything gs_debug_upload_plan answers for the inputs `i` (upload_plan_cases.make_inputs)."""
    before = Bitmap(i["ranges"])
    held = Bitmap(i["ranges"]).holding(i["hold_from"], i["hold_count"])
    out = {"segments": plan_upload(i["ranges"], i["from"], i["count"], i["reorder"]), "before": before.runs(),
           "after": ranges_after(i["ranges"], i["from"], i["count"]), "held": held}
    out.update(upload_layout(i["layout_count"], i["cov_half"], i["mesh_sh_u8"], i["sh_degree"], i["source_stages_sh_u8"]))
    return out
