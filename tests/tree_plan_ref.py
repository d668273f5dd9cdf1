"""Host model (numpy) of the octree gather's plan - csrc/tree.hip: k_tree_test, k_tree_scan, k_tree_fill, k_tree_offsets and the
copy - WITH its state: key, hist, start, fill, chunk_sum, members and prev_scale live in the model object and are carried from
gather to gather exactly as the device carries them in the tree (fill is reset by the NEXT gather's k_tree_test from the previous
keys and prev_scale; hist is zeroed by k_tree_fill).  Integer arithmetic is the kernels' (packed members << 40 | splats words,
uint32 offsets that wrap); the fp64 key is evaluated in the operation order of tree_leaf_key (numpy never contracts).

The order in which the leaves of one bucket take their member slots (an atomicAdd on the device: arbitrary) follows a seeded
permutation.  The model reports writes outside its arrays instead of making them.

MUTATIONS (one switch each; tests/test_tree_plan_ref.py shows that the case list catches every one):
  m1   the member loop stops after the first batch of 8
  m2   the tie-break on the leaf number is dropped
  m3   own-bucket members are compared by bucket only (the key is ignored: leaf number alone)
  m4   padding lanes add their count
  m5   fill is never reset
  m6   fill is reset with the current scale instead of prev_scale
  m7   hist is not zeroed after the fill
  m8   the chunk base is left out of first / before
  m9   before is weighted by members instead of splats
  m10  the clamp of tree_bucket is missing (the index wraps to b mod 2^18)
"""
import math

import numpy as np

from tree_plan_cases import host_scale

TREE_BUCKETS = 1 << 18
PLAN_GRID = 256
PLAN_CHUNK = TREE_BUCKETS // PLAN_GRID
W_MASK = (1 << 40) - 1
INF_BITS = np.uint64(0x7FF0000000000000)
CULLED = 0xFFFFFFFF
POISON = np.uint32(0xFFFFFFFF)            # list slots no leaf wrote
MUTATIONS = ("m1", "m2", "m3", "m4", "m5", "m6", "m7", "m8", "m9", "m10")


class PlanModel:
    def __init__(self, leaves, scene_min, scene_max, member_seed=0, mutation=None):
        """leaves: oracle/tree_oracle.py::build_tree's; scene_min / scene_max: the box of the uploaded fp32 centres."""
        assert mutation is None or mutation in MUTATIONS
        self.mut = mutation
        L = self.L = len(leaves)
        self.center = np.array([lf["center"] for lf in leaves], np.float64).reshape(L, 3)
        d = np.array([[lf["max"][k] - lf["min"][k] for k in range(3)] for lf in leaves], np.float64).reshape(L, 3)
        self.size = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        self.count = np.array([len(lf["indexes"]) for lf in leaves], np.int64)
        self.lists = [np.asarray(lf["indexes"], np.uint32) for lf in leaves]
        self.splats = int(self.count.sum())
        self.scene_min, self.scene_max = np.asarray(scene_min, np.float64), np.asarray(scene_max, np.float64)
        self.rng = np.random.default_rng(member_seed)
        # device state (gs_tree_create: tables zero, keys +inf = "no previous gather")
        self.key = np.full(L, INF_BITS, np.uint64)
        self.hist = np.zeros(TREE_BUCKETS, np.uint64)
        self.start = np.zeros(TREE_BUCKETS, np.uint64)
        self.fill = np.zeros(TREE_BUCKETS, np.int64)
        self.chunk_sum = np.zeros(PLAN_GRID, np.uint64)
        self.members = np.zeros(L, np.int64)
        self.offset = np.full(L, CULLED, np.int64)
        self.prev_scale = 1.0
        self.oob = []                         # what the last gather would have written outside its arrays

    # tree_bucket over an array of finite keys >= 0
    def _bucket(self, key, scale):
        b = key * scale
        if self.mut == "m10":
            return np.where(b < 1e18, np.fmod(np.floor(np.minimum(b, 1e18)), float(TREE_BUCKETS)), 0.0).astype(np.int64)
        return np.where(b < float(TREE_BUCKETS - 1), np.minimum(b, float(TREE_BUCKETS)), float(TREE_BUCKETS - 1)).astype(np.int64)

    def _keys(self, mv, fov, width, height, gather_all):
        """tree_leaf_key per leaf: fp64 distance, +inf when culled"""
        e = [float(v) for v in mv]
        deg2rad = 3.14159265358979323846 / 180.0
        focal = (height / 2.0) / math.tan(fov / 2.0 * deg2rad)
        thr_x = math.cos(math.atan(width / 2.0 / focal)) - .6
        thr_y = math.cos(math.atan(height / 2.0 / focal)) - .6
        x, y, z = self.center[:, 0], self.center[:, 1], self.center[:, 2]
        with np.errstate(all="ignore"):
            w = 1.0 / (e[3] * x + e[7] * y + e[11] * z + e[15])
            vx = (e[0] * x + e[4] * y + e[8] * z + e[12]) * w
            vy = (e[1] * x + e[5] * y + e[9] * z + e[13]) * w
            vz = (e[2] * x + e[6] * y + e[10] * z + e[14]) * w
            dist = np.sqrt(vx * vx + vy * vy + vz * vz)
            s = 1.0 / np.where(dist != 0.0, dist, 1.0)
            vx, vy, vz = vx * s, vy * s, vz * s
            lyz = np.sqrt(0.0 * 0.0 + vy * vy + vz * vz)
            yz_z = vz * (1.0 / np.where(lyz != 0.0, lyz, 1.0))
            lxz = np.sqrt(vx * vx + 0.0 * 0.0 + vz * vz)
            xz_z = vz * (1.0 / np.where(lxz != 0.0, lxz, 1.0))
            out_y, out_x = -yz_z < thr_y, -xz_z < thr_x
            skip = (out_x | out_y) & (dist > self.size)
        if gather_all:
            skip = np.zeros(self.L, bool)
        return np.where(skip, np.inf, dist)

    def gather(self, model_view, fov, width, height, gather_all=False):
        """One gs_tree_gather.  Returns dict(list uint32 [total], total, kept, offset int64 [L], oob [str])."""
        L, mut = self.L, self.mut
        self.oob = []
        mv = np.asarray(model_view, np.float64).reshape(16)
        scale = host_scale(self.scene_min, self.scene_max, mv)
        # ---- k_tree_test: the previous gather's member counters go back to zero, then the keys and the bucket counters
        old_kept = self.key != INF_BITS
        if mut != "m5" and old_kept.any():
            self.fill[self._bucket(self.key[old_kept].view(np.float64), scale if mut == "m6" else self.prev_scale)] = 0
        k = self._keys(mv, float(fov), float(width), float(height), gather_all)
        self.key = k.view(np.uint64).copy()
        kept = self.key != INF_BITS
        kept_ids = np.flatnonzero(kept)
        bucket = np.zeros(L, np.int64)
        bucket[kept] = self._bucket(k[kept], scale)
        np.add.at(self.hist, bucket[kept], (np.uint64(1) << np.uint64(40)) | self.count[kept].astype(np.uint64))
        # ---- k_tree_scan: exclusive scan inside every chunk of 1024 buckets (both fields at once), chunk totals
        h = self.hist.reshape(PLAN_GRID, PLAN_CHUNK)
        incl = np.cumsum(h, axis=1, dtype=np.uint64)
        self.start = (incl - h).reshape(-1)
        self.chunk_sum = incl[:, -1].copy()
        # ---- chunk bases (plan_chunk_bases)
        base = np.cumsum(self.chunk_sum, dtype=np.uint64) - self.chunk_sum
        total_word = int(self.chunk_sum.sum(dtype=np.uint64))
        if mut == "m8":
            base = np.zeros(PLAN_GRID, np.uint64)
        # ---- k_tree_fill: members[first + fill++] = leaf, in an arbitrary (here: seeded) order; hist back to zero
        for i in self.rng.permutation(kept_ids):
            b = int(bucket[i])
            first = (int(base[b // PLAN_CHUNK]) + int(self.start[b])) >> 40
            slot = (first + int(self.fill[b])) & 0xFFFFFFFF
            self.fill[b] += 1
            if slot < L:
                self.members[slot] = i
            else:
                self.oob.append("members[%d] of %d (leaf %d)" % (slot, L, i))
        if mut != "m7":
            self.hist[bucket[kept]] = 0
        # ---- k_tree_offsets
        total = total_word & W_MASK & 0xFFFFFFFF
        kept_count = (total_word >> 40) & 0xFFFFFFFF
        self.offset = np.full(L, CULLED, np.int64)
        order = kept_ids[np.argsort(bucket[kept_ids], kind="stable")]
        edges = np.flatnonzero(np.diff(bucket[order])) + 1
        for ids in np.split(order, edges) if len(order) else []:     # the leaves of one bucket: one row each, same member list
            b = int(bucket[ids[0]])
            at = int(base[b // PLAN_CHUNK]) + int(self.start[b])
            lo, n = at >> 40, int(self.fill[b])
            before0 = (at >> 40) if mut == "m9" else (at & W_MASK)
            if mut == "m1":
                n = min(n, 8)
            padded = -(-n // 8) * 8                          # batches of 8
            pos = lo + np.arange(padded)
            real = np.arange(padded) < n
            if (pos[real] >= L).any():
                self.oob.append("members[%d:%d] of %d read by bucket %d" % (lo, lo + n, L, b))
            mem = self.members[np.minimum(pos, L - 1)]
            m = np.where(real[None, :], mem[None, :], ids[:, None])              # padding = the leaf itself: adds 0
            km, cm = self.key[m], self.count[m]
            if mut == "m9":
                cm = np.ones_like(cm)
            mine = self.key[ids][:, None]
            if mut == "m2":
                first_ = km < mine
            elif mut == "m3":
                first_ = m < ids[:, None]
            else:
                first_ = (km < mine) | ((km == mine) & (m < ids[:, None]))
            if mut == "m4":
                first_ = first_ | ~real[None, :]
            before = before0 + (cm * first_).sum(axis=1)
            self.offset[ids] = (total - (before & 0xFFFFFFFF) - self.count[ids]) & 0xFFFFFFFF
        self.prev_scale = scale
        # ---- k_tree_copy: every kept leaf's index list to its offset
        size = min(total, 4 * self.splats + 16)              # (a mutated total may exceed the tree: the comparison fails anyway)
        out = np.full(size, POISON, np.uint32)
        for i in kept_ids:
            o, c = int(self.offset[i]), int(self.count[i])
            if o + c > self.splats:                          # the destination holds the tree's splats
                self.oob.append("list[%d:%d] of %d (leaf %d)" % (o, o + c, self.splats, i))
            if o + c <= size:
                out[o:o + c] = self.lists[i]
        return dict(list=out, total=total, kept=kept_count, offset=self.offset.copy(), oob=list(self.oob), scale=scale)
