"""The host-side planning of the keypoint pool and the window store
(form_amd/csrc/store_plan.hpp) without a device: random sequences of add / remove / persist
driven through tests/cpp/test_store_plan (the header under the address and
undefined-behaviour sanitizers) and, step by step, through the restatements in
tests/store_ref.py.  The planned copies are applied to numpy buffers; after every step the
buffers hold what the restatement holds, at the offsets the plan reports."""
import os
import subprocess

import numpy as np
import pytest

import store_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "tests", "cpp", "test_store_plan")
NONE = -1  # a buffer element nothing was written to


def _need_prog():
    assert os.path.exists(PROG), "tests/cpp/test_store_plan is not built (__graft_entry__.build())"


def test_fixed_cases_under_sanitizers():
    _need_prog()
    r = subprocess.run([PROG], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "store_plan ok", (r.returncode, r.stdout, r.stderr[-2000:])


class _Drive:
    def __init__(self):
        _need_prog()
        self.p = subprocess.Popen([PROG, "drive"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def __call__(self, *words):
        self.p.stdin.write(" ".join(str(w) for w in words) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        assert line, "the planning program ended: exit status %r" % self.p.poll()
        head, state = line.split("|")
        return head.split(), [int(x) for x in state.split()]

    def close(self):
        self.p.stdin.close()
        assert self.p.wait(timeout=60) == 0


def _copies(words, n):
    v = [int(x) for x in words[:3 * n]]
    return [tuple(v[3 * k:3 * k + 3]) for k in range(n)], words[3 * n:]


def _apply(src, dst, copies, src_cap):
    """Copy (src offset, dst offset, length) blocks; no two may overlap in the destination, all
    stay inside both buffers."""
    taken = np.zeros(len(dst), bool)
    for s, d, n in copies:
        assert 0 <= s and s + n <= src_cap and 0 <= d and d + n <= len(dst), (s, d, n, src_cap, len(dst))
        assert not taken[d:d + n].any(), ("copies overlap in the destination", s, d, n)
        taken[d:d + n] = True
        dst[d:d + n] = src[s:s + n]


# ------------------------------------------------------------------ keypoint pool
@pytest.mark.parametrize("seed,limit", [(0, 1000), (1, 257), (2, 64)])
def test_pool_random_sequences(seed, limit):
    g = np.random.default_rng(seed)
    alloc = limit + 100  # the limit lies below the allocated size
    drive = _Drive()
    drive("P", limit, alloc)
    ref = SR.PoolRef(limit)
    buf = np.full(alloc, NONE, np.int64)
    next_rec, next_scan, last = 0, 0, None
    seen = dict(ok=0, oom=0, state=0, compacted=0, exact=0, one_over=0, whole=0)
    for step in range(400):
        kind = g.choice(["add", "add", "add", "more", "remove", "exact", "over", "whole"])
        live_scans = ref.scans()
        added = not (kind == "remove" and live_scans)
        if not added:
            s = int(g.choice(live_scans))
            ref.remove(s)
            head, st = drive("r", s)
            status, compacted, copies = "ok", False, []
        else:
            room, room_c = limit - ref.tail, limit - ref.live
            if kind == "exact":  # fills the pool to the last record, as stored or once compacted
                n = room if room > 0 and g.random() < 0.5 else room_c
                seen["exact"] += 1
            elif kind == "over":  # one more than fits, as stored or even compacted
                n = (room if g.random() < 0.5 else room_c) + 1
                seen["one_over"] += 1
            elif kind == "whole":  # larger than the whole pool
                n = limit + int(g.integers(1, 50))
                seen["whole"] += 1
            else:
                n = int(g.integers(0, max(limit // 4, 2)))
            # "more": append to an existing scan (legal only for the last one stored)
            s = int(g.choice(live_scans)) if kind == "more" and live_scans and g.random() < 0.5 else \
                last if kind == "more" and last in live_scans else next_scan
            next_scan += s == next_scan
            recs = list(range(next_rec, next_rec + n))
            next_rec += n
            status, compacted = ref.add(s, recs)
            head, st = drive("a", s, n)
            assert head[0] == status and int(head[1]) == compacted, (step, kind, s, n, head, status, compacted)
            copies, rest = _copies(head[3:], int(head[2]))
            assert not rest
            if compacted:
                nbuf = np.full(alloc, NONE, np.int64)
                _apply(buf, nbuf, copies, alloc)
                buf = nbuf
            else:
                assert not copies
            seen[status] += 1
            seen["compacted"] += compacted
            if status == "ok":
                last = s
        used, nr = st[0], st[1]
        ranges = {st[2 + 3 * k]: (st[3 + 3 * k], st[4 + 3 * k]) for k in range(nr)}
        if added and status == "ok" and n:
            off, cnt = ranges[s]
            buf[off + cnt - n:off + cnt] = recs  # the upload the caller does at the old fill mark
        # the buffer holds the restatement, live and removed blocks alike, up to the fill mark
        assert used == ref.tail <= limit, (step, used, ref.tail)
        assert buf[:used].tolist() == ref.layout(), step
        assert sorted(k for k, v in ranges.items() if v[1]) == sorted(ref.scans()), step
        for sc in ref.scans():
            off, cnt = ranges[sc]
            assert off + cnt <= used and buf[off:off + cnt].tolist() == ref.records(sc), (step, sc)
    drive.close()
    assert ref.compactions == seen["compacted"] >= 20, seen
    assert min(seen.values()) > 0, seen  # every kind of request and every outcome occurred


# ------------------------------------------------------------------ window store
def _win_state(st):
    cap, tail, alloc, cur, ns = st[0:2], st[2:4], st[4:8], st[8], st[9]
    segs, k = {}, 10
    for _ in range(ns):
        j, plo, pto, pln, ptn, npairs = st[k:k + 6]
        k += 6
        pairs = [tuple(st[k + 5 * q:k + 5 * q + 5]) for q in range(npairs)]
        k += 5 * npairs
        segs[j] = dict(off=(plo, pto), n=(pln, ptn), pairs=pairs)
    assert k == len(st)
    return cap, tail, alloc, cur, segs


@pytest.mark.parametrize("seed,caps", [(0, (512, 128)), (1, (64, 4096)), (2, (4096, 32)), (3, (100, 25))])
def test_window_store_random_sequences(seed, caps):
    """caps: both arenas small; a small plane arena beside a roomy point arena and the reverse (a
    compaction then grows one and only compacts the other); capacities that are no power of two."""
    g = np.random.default_rng(10 + seed)
    drive = _Drive()
    drive("W", 0, caps[0], caps[1])
    ref = SR.WinRef(*caps)
    arena = [[np.full(c, NONE, np.int64) for _ in range(2)] for c in caps]  # [type][ping-pong]
    cur = 0
    next_row, j = [0, 0], 0
    seen = dict(compacted=0, grew_pl=0, grew_pt=0, exact=0, one_over=0, whole=0, removed=0)
    for step in range(300):
        kind = g.choice(["persist", "persist", "persist", "remove", "remove", "exact", "over", "whole"])
        alive = [s["j"] for s in ref.alive()]
        if len(alive) > 6:  # a bounded window, as in the estimator
            kind = "remove"
        if kind == "remove" and alive:
            s = int(g.choice(alive))
            ref.remove(s)
            head, st = drive("e", s)
            seen["removed"] += 1
        else:
            t = int(g.integers(0, 2))  # the row type the edge case is about
            n = [int(g.integers(0, max(ref.cap[u] // 10, 2))) for u in range(2)]
            if ref.cap[t] >= 20000:  # (each edge case can double the arena: no more of them)
                pass
            elif kind == "exact":  # to the last row of the arena as stored
                n[t] = max(ref.cap[t] - ref.tail(t), 0)
                seen["exact"] += 1
            elif kind == "over":
                n[t] = ref.cap[t] - ref.tail(t) + 1
                seen["one_over"] += 1
            elif kind == "whole":  # more rows than the whole arena
                n[t] = ref.cap[t] + int(g.integers(1, 9))
                seen["whole"] += 1
            # split among map scans, some of them without rows, one possibly unknown to the store
            ids = sorted(set(int(x) for x in g.choice(alive + [1000 + step], min(len(alive) + 1, 4), replace=False)))
            parts = []
            for q, i in enumerate(ids):
                cnt = [n[u] // len(ids) + (n[u] % len(ids) if q == 0 else 0) for u in range(2)]
                if g.random() < 0.2 and q:
                    cnt = [0, 0]
                rows = []
                for u in range(2):
                    rows.append(list(range(next_row[u], next_row[u] + cnt[u])))
                    next_row[u] += cnt[u]
                parts.append((i, rows[0], rows[1]))
            j += 1
            compacted, gpl, gpt = ref.persist(j, parts)
            words = ["p", j, len(parts)]
            for p in parts:
                words += [p[0], len(p[1]), len(p[2])]
            head, st = drive(*words)
            assert [int(x) for x in head[1:4]] == [compacted, gpl, gpt], (step, head[:5], compacted, gpl, gpt)
            nc = int(head[4])
            cpl, rest = _copies(head[5:], nc)
            cpt, rest = _copies(rest, nc)
            assert not rest
            if compacted:
                for u, copies in enumerate((cpl, cpt)):
                    src = arena[u][cur]
                    if len(arena[u][1 - cur]) < ref.cap[u]:  # grown: the destination arena first ...
                        arena[u][1 - cur] = np.full(ref.cap[u], NONE, np.int64)
                    dst = arena[u][1 - cur]
                    dst[:] = NONE
                    _apply(src, dst, copies, len(src))
                    if len(src) < ref.cap[u]:  # ... then the old one (free space only)
                        arena[u][cur] = np.full(ref.cap[u], NONE, np.int64)
                cur = 1 - cur
                # after a growth the live rows fill at most half of the arena
                if gpl:
                    assert 2 * (ref.live(0)) <= ref.cap[0]
                if gpt:
                    assert 2 * (ref.live(1)) <= ref.cap[1]
            else:
                assert nc == 0
            seen["compacted"] += compacted
            seen["grew_pl"] += gpl
            seen["grew_pt"] += gpt
        cap, tail, alloc, pcur, segs = _win_state(st)
        if kind != "remove" or not alive:
            # the caller's copy of the new segment's rows to the tail
            sg = segs[j]
            for u in range(2):
                arena[u][cur][sg["off"][u]:sg["off"][u] + sg["n"][u]] = [r for p in parts for r in p[1 + u]]
        assert cap == ref.cap and pcur == cur, (step, cap, ref.cap)
        for u, width in enumerate((9, 6)):
            assert tail[u] == ref.tail(u) <= cap[u], (step, u, tail, ref.tail(u), cap)
            assert min(alloc[2 * u:2 * u + 2]) >= width * cap[u]  # both arenas hold the capacity
            assert arena[u][cur][:tail[u]].tolist() == ref.layout(u), (step, u)
        assert sorted(segs) == [s["j"] for s in ref.alive()], step
        for s in ref.alive():
            sg = segs[s["j"]]
            assert [p[0] for p in sg["pairs"]] == [p["i"] for p in s["pairs"]], (step, s["j"])
            for u in range(2):
                assert sg["off"][u] + sg["n"][u] <= tail[u]
                assert arena[u][cur][sg["off"][u]:sg["off"][u] + sg["n"][u]].tolist() == s["rows"][u], (step, s["j"])
            for got, want in zip(sg["pairs"], s["pairs"]):
                for u in range(2):
                    off, cnt = got[1 + u], got[3 + u]
                    assert sg["off"][u] <= off and off + cnt <= sg["off"][u] + sg["n"][u], (step, got)
                    assert arena[u][cur][off:off + cnt].tolist() == want["rows"][u], (step, s["j"], got)
    drive.close()
    assert ref.compactions == seen["compacted"] >= 10, seen
    assert min(seen.values()) > 0, seen  # every kind of request and both growths occurred


def test_production_sizes_without_limits():
    """No limits: the first reservation asks for max(keypoint_pool_capacity, 2^20) plane rows
    and a quarter of that for point rows, and the store adopts what the buffers over-allocate."""
    drive = _Drive()
    head, st = drive("W", 4 << 20, 0, 0)
    head, st = drive("p", 1, 1, 0, 25000, 100)
    cap, tail, alloc, cur, segs = _win_state(st)
    a_pl, a_pt = 2 * 9 * (4 << 20) + 64, 2 * 6 * (1 << 20) + 64
    assert alloc == [a_pl, a_pl, a_pt, a_pt] and cap == [a_pl // 9, a_pt // 6]
    assert head[:4] == ["ok", "0", "0", "0"] and tail == [25000, 100] and cur == 0
    head, st = drive("W", 100, 0, 0)
    head, st = drive("p", 1, 1, 0, 5, 5)
    cap, tail, alloc, cur, segs = _win_state(st)
    assert cap == [(2 * 9 * (1 << 20) + 64) // 9, (2 * 6 * (1 << 18) + 64) // 6]
    drive.close()
