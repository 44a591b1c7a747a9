"""Plain restatements of the two stores that move their contents: the keypoint pool
(fmx_api.cpp: pool_add / ensure_pool_room / compact_pool) and the smoothing-mode window store
(window.hip: win_persist / win_reserve / win_remove).  They act on the stored values
themselves: a pool is a list of blocks of records, a window store a list of segments with
their pairs' rows; nothing here keeps an offset.  tests/test_store_cpu.py holds the planning
header (form_amd/csrc/store_plan.hpp) to them, tests/test_gpu_store.py the device."""


class PoolRef:
    """One feature type's pool under a record limit.  Storage is the sequence of blocks
    appended since the last compaction, removed ones included (they take room until then)."""

    def __init__(self, limit):
        self.limit = int(limit)
        self.blocks = []  # [scan, [records...], alive]
        self.compactions = 0

    @property
    def tail(self):
        return sum(len(b[1]) for b in self.blocks)

    @property
    def live(self):
        return sum(len(b[1]) for b in self.blocks if b[2])

    def scans(self):
        return [b[0] for b in self.blocks if b[2]]

    def records(self, scan):
        for b in self.blocks:
            if b[2] and b[0] == scan:
                return b[1]
        return []

    def add(self, scan, records, need=None):
        """-> (status, compacted): "ok", "oom" (does not fit even compacted; the compaction
        stays) or "state" (the scan's earlier records are no longer last).  need: the room
        asked for when it is more than the records (insert_matches asks for every query's)."""
        records = list(records)
        need = len(records) if need is None else need
        if not need:
            return "ok", False
        compacted = False
        if self.tail + need > self.limit:
            self.blocks = [b for b in self.blocks if b[2]]
            self.compactions += 1
            compacted = True
            if self.tail + need > self.limit:
                return "oom", True
        if not records:
            return "ok", compacted
        mine = [b for b in self.blocks if b[2] and b[0] == scan]
        if mine:
            if self.blocks[-1] is not mine[0]:
                return "state", compacted
            mine[0][1].extend(records)
        else:
            self.blocks.append([scan, records, True])
        return "ok", compacted

    def remove(self, scan):
        for b in self.blocks:
            if b[0] == scan:
                b[2] = False

    def layout(self):
        """Every stored record in storage order, removed blocks included."""
        return [r for b in self.blocks for r in b[1]]


class WinRef:
    """The window store with exact capacities (the test limits): segments of plane and point
    rows, each split among its pairs (i, j).  A compaction keeps the live segments, j
    ascending, and doubles a capacity until the live rows, the new ones included, fill at
    most half of it."""

    def __init__(self, cap_pl, cap_pt):
        self.cap = [int(cap_pl), int(cap_pt)]
        self.segs = []  # dict(j, rows=[pl rows, pt rows], pairs=[dict(i, rows=[pl, pt])], alive)
        self.compactions = 0
        self.growths = [0, 0]

    def tail(self, t):
        return sum(len(s["rows"][t]) for s in self.segs)

    def live(self, t):
        return sum(len(s["rows"][t]) for s in self.segs if s["alive"])

    def alive(self):
        return sorted((s for s in self.segs if s["alive"]), key=lambda s: s["j"])

    def persist(self, j, parts):
        """parts: [(i, plane rows, point rows)] in map-scan order; pairs without rows are not
        kept.  -> (compacted, grew plane, grew point)"""
        n = [sum(len(p[1 + t]) for p in parts) for t in range(2)]
        out = (False, False, False)
        if any(self.tail(t) + n[t] > self.cap[t] for t in range(2)):
            grew = [False, False]
            for t in range(2):
                while 2 * (self.live(t) + n[t]) > self.cap[t]:
                    self.cap[t] *= 2
                    grew[t] = True
                self.growths[t] += grew[t]
            self.segs = self.alive()
            self.compactions += 1
            out = (True, grew[0], grew[1])
        for s in self.segs:
            if s["j"] == j:
                s["alive"] = False  # replaced: its rows stay until the next compaction
        self.segs.append(dict(j=j, alive=True, rows=[[r for p in parts for r in p[1 + t]] for t in range(2)],
                              pairs=[dict(i=p[0], rows=[list(p[1]), list(p[2])]) for p in parts
                                     if len(p[1]) + len(p[2]) > 0]))
        return out

    def remove(self, scan):
        for s in self.segs:
            if s["j"] == scan:
                s["alive"] = False
            s["pairs"] = [p for p in s["pairs"] if p["i"] != scan]

    def layout(self, t):
        return [r for s in self.segs for r in s["rows"][t]]
