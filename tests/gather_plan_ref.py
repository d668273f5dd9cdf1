"""Host models of csrc/gather_plan.cpp, written from the reference's expressions and from the rules, not from the library.

plan       the two cull thresholds of Viewer.gatherSceneNodesForSort (src/Viewer.js:1990-1996, as oracle/tree_oracle.py::gather states
           them), the bucket scale from the farthest scene-box corner (plain + - * / sqrt in Python floats = IEEE doubles, every
           operation rounded once), and the policy words.
hand-over  what a gather leaves a sorter: one of three states per sorter.  The tree's back-pointer is not stored here at all - it
           is derived from the sorters' states, so the library's stored pointer is held to the invariant by every comparison."""
import math

TREE_BUCKETS = 1 << 18
PLAN_THREADS = 256
MAX_SCENES = 32
SORT_DYNAMIC = 2

# ------------------------------------------------------------------------------------------------------------------- the plan


def thresholds(fov_y_deg, render_w, render_h):
    focal = (render_h / 2.0) / math.tan(fov_y_deg / 2.0 * (math.pi / 180.0))
    cos_x = math.cos(math.atan(render_w / 2.0 / focal))
    cos_y = math.cos(math.atan(render_h / 2.0 / focal))
    return cos_x - .6, cos_y - .6


def corner_distances(scene):
    """Distance of the 8 box corners from the eye under the scene's modelView (Vector3.applyMatrix4, a zero w counts as 1)."""
    mn, mx, e = scene["box"][:3], scene["box"][3:], scene["model_view"]
    out = []
    for c in range(8):
        x = mx[0] if c & 1 else mn[0]
        y = mx[1] if c & 2 else mn[1]
        z = mx[2] if c & 4 else mn[2]
        w = e[3] * x + e[7] * y + e[11] * z + e[15]
        w = 1.0 / w if w != 0.0 else 1.0
        vx = (e[0] * x + e[4] * y + e[8] * z + e[12]) * w
        vy = (e[1] * x + e[5] * y + e[9] * z + e[13]) * w
        vz = (e[2] * x + e[6] * y + e[10] * z + e[14]) * w
        out.append(math.sqrt(vx * vx + vy * vy + vz * vz))
    return out


def all_corner_distances(i):
    return [d for s in i["scenes"] if not s["empty"] for d in corner_distances(s)]


def bucket_scale(i):
    far = 0.0
    for d in all_corner_distances(i):
        if d > far:
            far = d
    return TREE_BUCKETS / (far * 1.0001) if 0.0 < far < 1e300 else 1.0


def gather_plan(i):
    thr_x, thr_y = thresholds(i["fov_y_deg"], i["render_width"], i["render_height"])
    scene_table = len(i["scenes"]) > 1
    deferred = bool(i["leaves"] and i["has_sorter"] and not i["host_copy"] and not (i["sorter_flags"] & SORT_DYNAMIC) and
                    not i["no_defer"] and not scene_table)
    zero_keep = deferred and bool(i["frustum_cull"])
    return dict(thr_x=thr_x, thr_y=thr_y, scale=bucket_scale(i), deferred=int(deferred), zero_keep=int(zero_keep),
                keep_words=(i["tree_splats"] + 63) // 64 + 2 if zero_keep else 0,
                leaf_grid=(i["leaves"] + PLAN_THREADS - 1) // PLAN_THREADS, scene_table=int(scene_table))


def buckets_in_range(i, scale):
    """Every leaf centre lies inside its scene's box, whose farthest corner bounds its distance: no finite corner distance may
    fall beyond the last bucket."""
    return all(math.floor(d * scale) <= TREE_BUCKETS - 1 for d in all_corner_distances(i) if math.isfinite(d))


def mat4_multiply(a, b):
    """Matrix4.multiplyMatrices (three r160), column-major."""
    return [a[r] * b[4 * c] + a[r + 4] * b[4 * c + 1] + a[r + 8] * b[4 * c + 2] + a[r + 12] * b[4 * c + 3] for c in range(4) for r in range(4)]


# --------------------------------------------------------------------------------------------------------------- the hand-over
NONE, PLANNED, COPIED = 0, 1, 2
EV_GATHER, EV_SORT_GATHERED, EV_SORT_OTHER, EV_TREE_DESTROYED, EV_SORTER_DESTROYED, EV_FORGET_NUMBERING, EV_MESH_REORDERED = range(7)
NOBODY = 2                                                 # no sorter (a host gather) / no tree
SORT_OK, SORT_NO_LIST, SORT_PARTIAL_ASYNC = 0, 1, 2


class Handover:
    """Two sorters; step(event) returns what the library's replay reports after the same event."""

    def __init__(self):
        self.s = [self.nothing(), self.nothing()]

    @staticmethod
    def nothing():
        return dict(state=NONE, tree=NOBODY, keep=0, count=0, dev=0)

    def planner(self, tree):
        who = [k for k, s in enumerate(self.s) if s["state"] == PLANNED and s["tree"] == tree]
        assert len(who) <= 1, "two sorters wait for one tree's tables"
        return who[0] if who else NOBODY

    def copied(self, k):                                   # the planned list is (or is about to be) in idx_in
        if self.s[k]["state"] == PLANNED:
            self.s[k].update(state=COPIED, tree=NOBODY, keep=0)

    def step(self, kind, tree=0, sorter=0, a=0, b=0, c=0, d=0):
        out = dict(evicted=NOBODY, refused=0, sort_count=0, render_count=0, sort_on_device=0)
        s = self.s[sorter] if sorter != NOBODY else None
        if kind == EV_GATHER:
            waiting = self.planner(tree)
            if waiting not in (NOBODY, sorter):            # the tree's tables are about to be overwritten: it copies now
                out["evicted"] = waiting
                self.copied(waiting)
            if s is not None:                              # (a plan of its own in another tree is superseded)
                s.update(state=PLANNED if a else COPIED, tree=tree if a else NOBODY, keep=int(bool(a and b)), count=c, dev=int(bool(d)))
        elif kind == EV_SORT_GATHERED:
            if s["state"] == NONE:
                out["refused"] = SORT_NO_LIST
            else:
                whole = s["count"]
                out.update(refused=SORT_PARTIAL_ASYNC if s["dev"] and a < whole else SORT_OK,
                           sort_count=whole if s["dev"] else min(a, whole), render_count=whole, sort_on_device=s["dev"])
                if out["refused"] == SORT_OK:
                    self.copied(sorter)
        elif kind == EV_SORT_OTHER:
            if b:                                          # a frustum-culled sort rewrites the keep mask
                s["keep"] = 0
            if (a or c) and s["state"] == COPIED:          # a host list / the compaction overwrites idx_in
                self.s[sorter] = self.nothing()
        elif kind == EV_TREE_DESTROYED:
            waiting = self.planner(tree)
            if waiting != NOBODY:
                self.s[waiting] = self.nothing()
        elif kind in (EV_SORTER_DESTROYED, EV_FORGET_NUMBERING):
            self.s[sorter] = self.nothing()
        else:
            assert kind == EV_MESH_REORDERED
        out.update(state=[s["state"] for s in self.s], tree_of=[s["tree"] for s in self.s], keep_zeroed=[s["keep"] for s in self.s],
                   count=[s["count"] for s in self.s], count_on_device=[s["dev"] for s in self.s],
                   planner=[self.planner(0), self.planner(1)])
        return out
