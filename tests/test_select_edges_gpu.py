"""hso_gpu_reproject_select (k_select, hso_amd/csrc/hso_select.hip) against the sequential walk of tests/test_select.py at the sizes
where its scans take a second trip: every stage of the kernel is a loop over chunks of SEL_THREADS = 1024 visiting indices with a
`carry` between the chunks, and each budget scan places its cut with an atomicMin.  The tables here have more than 1024 cells or
candidates, cuts on and next to the chunk boundaries, cells whose packed fields (e1 / e2 bits 30 and 29, a3 = successes clamped to a
byte | length << 8) are at their limits, and the smallest grids and budgets.

Every comparison is exact: the examined list (index, taken) in order, counts[0:3] == (len, n_matches, passes), counts[3] == branch.
The CPU half (test_tables_aim_where_they_say) shows on the sequential walk alone that every hand-built table ends in the pass, at the
cell and with the number of features it was built for, so that the GPU half cannot aim beside its target."""
import numpy as np
import pytest

from test_select import make_frame, select_reference

CHUNK = 1024                                            # SEL_THREADS
JUNK = np.array([0, 2, 3], np.uint8)                    # not matched; deleted; matched and deleted (a trial, never a feature)
EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.uint8))


def order_for(n_cells):
    """the visiting order of a grid size: a permutation of its own per n_cells"""
    return np.random.default_rng(1000 + n_cells).permutation(n_cells).astype(np.int32)


def hand_table(rng, order, matched, junk, qmode="random"):
    """A frame from per-visit counts: the cell visited k-th (order[k]) holds matched[k] candidates with flags 1 and junk[k] with flags
    0 / 2 / 3, shuffled inside the cell.  Projection order deals the cells' candidates round by round, the cells of a round in random
    order: a cell's list lies scattered over the table and keeps its order.  qmode: the quality keys —
    equal (ties keep projection order), increasing (strictly, with projection order inside a cell: the sort reverses the cell),
    two (a mix of two values), random (point type << 4 | feature type as the engine forms them)."""
    matched = np.asarray(matched, np.int64); junk = np.asarray(junk, np.int64)
    cnt = matched + junk
    per = []
    for k in range(len(order)):
        f = np.concatenate([np.ones(matched[k], np.uint8), rng.choice(JUNK, junk[k])])
        rng.shuffle(f)
        per.append(f)
    k_of = np.repeat(np.arange(len(order)), cnt)
    j_of = np.concatenate([np.arange(c) for c in cnt])              # position inside the cell
    deal = np.argsort(j_of + rng.random(len(j_of)), kind="stable")
    flags = np.concatenate(per)[deal]
    cell = order[k_of][deal]
    n = len(cell)
    if qmode == "equal":
        quality = np.full(n, (3 << 4) | 1)
    elif qmode == "increasing":
        assert cnt.max() < 200
        quality = 16 + j_of[deal]
    elif qmode == "two":
        quality = rng.choice([(2 << 4) | 1, (4 << 4) | 2], n)
    else:
        quality = (rng.integers(1, 5, n) << 4) | rng.integers(0, 3, n)
    return cell.astype(np.int32), quality.astype(np.uint8), flags.astype(np.uint8)


def pass_gains(matched):
    """What each pass takes per visiting index when no pass is cut short (src/reprojector.cpp:268-305): one in pass 1, one more in
    pass 2 (which never visits index 0), up to three of the rest in pass 3.  Only used to PLACE a budget; the CPU half checks the
    placement against select_reference."""
    matched = np.asarray(matched, np.int64)
    g1 = (matched >= 1).astype(np.int64)
    g2 = (matched >= 2).astype(np.int64); g2[0] = 0
    return g1, g2, np.minimum(matched - g1 - g2, 3)


class Case:
    """frames that share one call: a grid, its visiting order and the budget.  A 37-candidate frame goes first (and before any
    frame that would start at a multiple of 64), an empty frame last: the ranges start at odd offsets and the call mixes branches."""

    def __init__(self, name, order, budget, frames, expect=None):
        self.name, self.order, self.budget = name, np.asarray(order, np.int32), int(budget)
        expect = list(expect) if expect is not None else [None] * len(frames)
        pad_rng = np.random.default_rng(sum(map(ord, name)))
        self.frames, self.expect, at = [], [], 0
        for fr, ex in zip(frames, expect):
            if at % 64 == 0:
                self.frames.append(make_frame(pad_rng, 37, len(self.order), 0.6, 0.1, False)); self.expect.append(None); at += 37
            self.frames.append(fr); self.expect.append(ex); at += len(fr[0])
        self.frames.append(EMPTY); self.expect.append(dict(passes=0, m=0, n_examined=0))
        self._refs = None

    def begins(self):
        return np.concatenate([[0], np.cumsum([len(f[0]) for f in self.frames])]).astype(np.int32)

    def refs(self):
        """the sequential walk per frame, computed once and shared by the CPU and the GPU half"""
        if self._refs is None:
            self._refs = []
            for cell, quality, flags in self.frames:
                out, m, passes = select_reference(cell, quality, flags, self.order, len(self.order), self.budget)
                self._refs.append(([(int(i), bool(t)) for i, t in out], m, passes))
        return self._refs

    def branch(self, k):
        """0 = reprojectCellAll (fewer than max_fts + 50 candidates; also what an empty frame or a zero budget reports), 1 = the cells"""
        n = len(self.frames[k][0])
        return int(n > 0 and self.budget > 0 and n >= self.budget + 50)


def ending(case, k):
    """how the walk of frame k ended, from the reference's return values alone"""
    _, m, passes = case.refs()[k]
    if case.branch(k) == 0:
        return "all"
    if passes == 3:
        return "pass 3" if m >= case.budget else "pass 3 ran out"
    return {1: "pass 1", 2: "passes 1 + 2"}[passes] if m >= case.budget else "?"


_CACHE = {}


def cached(fn):
    def get():
        if fn.__name__ not in _CACHE:
            _CACHE[fn.__name__] = fn()
        return _CACHE[fn.__name__]
    get.__name__ = fn.__name__
    return get


# ---------------------------------------------------------------------------------------------------------------- the tables
GRIDS = (1, 2, 1023, 1024, 1025, 2048, 2049, 5700)      # cells: 1 (pass 2 visits nothing), 2, both sides of one and two chunks of the
                                                        # cnt prefix (n_cells + 1 entries: hso_select.hip:123-131) and of every pass'
                                                        # scans (:78-89, :168-180, :192-205, :224-242), and the engine's grid


def two_per_cell(rng, order):
    """the pass-2 ending does not arise from random tables: two matched candidates in most cells, one in the others, a little junk —
    with a budget between n_cells and 2 n_cells pass 1 takes one per cell and pass 2 meets the budget"""
    nc = len(order)
    return hand_table(rng, order, np.where(rng.random(nc) < 0.9, 2, 1), rng.integers(0, 2, nc))


@cached
def grid_cases():
    cases = []
    for nc in GRIDS:
        rng = np.random.default_rng(7000 + nc)
        order = order_for(nc)
        if nc <= 2:
            frames = [make_frame(rng, 120, nc, 0.8, 0.05, False), make_frame(rng, 90, nc, 0.3, 0.1, False),
                      make_frame(rng, 70, nc, 0.1, 0.3, False), two_per_cell(rng, order)]
            budgets = (1, 2, 3, 4, 5, 8, 9, 20)
        else:
            frames = [make_frame(rng, 4 * nc, nc, 0.3, 0.05, False),        # 1.2 matches per cell: pass 3 runs out at 1.5 n_cells and above
                      make_frame(rng, 6 * nc, nc, 0.8, 0.03, False),        # 4.8 per cell: pass 3 meets 2 n_cells and 3 n_cells
                      make_frame(rng, 3 * nc, nc, 0.6, 0.05, True),         # a sixth of the cells hold everything
                      two_per_cell(rng, order),                             # passes 1 + 2 meet 1.5 n_cells
                      make_frame(rng, nc // 2, nc, 0.7, 0.05, False)]       # fewer than budget + 50 at the larger budgets: reprojectCellAll
            budgets = (nc // 4, nc + nc // 2, 2 * nc, 3 * nc)
        for b in budgets:
            cases.append(Case("grid %d budget %d" % (nc, b), order, b, frames))
    return cases


def cut_table(nc, which, k, take=0, rest=None, qmode="random", seed=0):
    """A table in which the budget is met exactly at index k of pass `which` (pass 2 counts its own index: j-th visited = order[nc-1-j]).
    Pass 3: the cut cell has `rest` successes left (default 5) and the budget runs out at the take-th of them."""
    rng = np.random.default_rng(seed + 31 * k + which)
    order = order_for(nc)
    matched = rng.integers(0, 7 if which == 3 else 4, nc)
    junk = rng.integers(1, 4, nc)
    if which == 1:
        at, matched[k] = k, max(matched[k], 1)
        g1, g2, g3 = pass_gains(matched)
        budget, taken_last = g1[:k + 1].sum(), 1
    elif which == 2:
        at = nc - 1 - k
        matched[at] = max(matched[at], 2)
        g1, g2, g3 = pass_gains(matched)
        budget, taken_last = g1.sum() + g2[at:].sum(), 2
    else:
        at = k
        matched[k] = (5 if rest is None else rest) + 1 + (1 if k > 0 else 0)
        g1, g2, g3 = pass_gains(matched)
        assert 1 <= take <= g3[k]
        budget, taken_last = g1.sum() + g2.sum() + g3[:k].sum() + take, g1[k] + g2[k] + take
    frame = hand_table(rng, order, matched, junk, qmode)
    assert len(frame[0]) >= budget + 50                 # the cell branch
    return frame, int(budget), dict(passes=which, m=int(budget), last_cell=int(order[at]), taken_last=int(taken_last))


@cached
def cut_cases():
    nc, cases = 2049, []
    def add(name, *a, **kw):
        frame, budget, ex = cut_table(nc, *a, **kw)
        small = make_frame(np.random.default_rng(budget), min(budget + 49, 300), nc, 0.7, 0.05, False)   # reprojectCellAll in the same call
        cases.append(Case(name, order_for(nc), budget, [frame, small], [ex, None]))
    for k in (CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, nc - 1):
        # pass 1 (hso_select.hip:163-164, the atomicMin at :85 with carry != 0): last index of chunk 0, first of chunk 1, their
        # neighbours; k = nc - 1: the budget is met by the LAST cell of pass 1 and no pass 2 may start (passes == 1, :184)
        add("pass 1 cut at %d" % k, 1, k, seed=100)
    for j in (CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, nc - 2):
        # pass 2 (:186-190): the index runs over cell_order[nc-1 .. 1], m = nc - 1; j = m - 1 is cell_order[1], the last cell of
        # pass 2: pass 3 must not start (passes == 2, :208)
        add("pass 2 cut at %d" % j, 2, j, seed=200)
    for k, take in ((CHUNK - 2, 1), (CHUNK - 1, 2), (CHUNK, 3), (CHUNK + 1, 1), (nc - 1, 2)):
        # pass 3 (:219-232): take = R - scan[k] needs the exclusive prefix of the SECOND chunk (scan[k] = incl - g with the carry added)
        add("pass 3 cut at %d take %d" % (k, take), 3, k, take=take, seed=300)
    for take in (1, 2, 3):
        # the cut inside a cell with five successes left, at its 1st, 2nd, 3rd (:231-232: ex = p3[take - 1])
        add("pass 3 take %d of 5" % take, 3, CHUNK + 7, take=take, seed=400 + take)
    for rest in (1, 2):
        # the cut on a cell with fewer than three successes: a3 < 3 and k == cut3 (:232 takes p3[take - 1], not len)
        add("pass 3 cut on a cell with %d left" % rest, 3, CHUNK + 9, take=rest, rest=rest, seed=500 + rest)
    # cell_order[0] holds two or more matched candidates: pass 2 skips it (:186), pass 3 starts behind pass 1's candidates only
    # (:212, bit 29 of e2 not set) and picks the rest up; the cut is in that very cell, at visiting index 0
    add("pass 3 cut at 0: cell_order[0]", 3, 0, take=2, seed=600)
    return cases


def heavy(rng, order, matched, junk, special, qmode):
    """a hand table in which the visiting indices in `special` = {k: (matched, junk)} are replaced"""
    matched, junk = np.array(matched), np.array(junk)
    for k, (m, j) in special.items():
        matched[k], junk[k] = m, j
    g1, g2, g3 = pass_gains(matched)
    return hand_table(rng, order, matched, junk, qmode), int(g1.sum() + g2.sum()), g3


@cached
def heavy_cases():
    """cells whose pass-3 record is at the limits of its packing (hso_select.hip:215: successes clamped to 255 | length << 8).  No
    cell holds more than 600 candidates: the per-cell insertion sort (:140-149) is serial."""
    nc, cases = 1025, []
    order = order_for(nc)
    rng = np.random.default_rng(77)
    light = rng.integers(0, 3, nc), rng.integers(1, 3, nc)
    # 600 candidates, all matched: 598 successes left for pass 3 (clamped to 255), len 598 >= 597
    f600, g12, g3 = heavy(rng, order, *light, {600: (600, 0)}, "equal")
    # 300 candidates of which none matches (e1 = 300 without bit 30, len 0 afterwards); 600 of which 514 match: 512 left = 0x200, whose
    # low byte is 0 — a one-byte count without the clamp reads "no success" here; 258 / 259 / 260 matched: 256 / 257 / 258 left
    fmix, g12m, g3m = heavy(rng, order, *light, {5: (0, 300), 300: (514, 86), 1023: (258, 3), 1024: (259, 0), 40: (260, 7)}, "two")
    for name, frame, base, g in (("600 matched", f600, g12, g3), ("512 and 256..258 left", fmix, g12m, g3m)):
        assert len(frame[0]) >= base + int(g.sum()) + 60
        cases.append(Case("heavy: %s, pass 3 runs out" % name, order, base + int(g.sum()) + 10, [frame]))
    cases.append(Case("heavy: 600 matched, cut at its 2nd", order, g12 + int(g3[:600].sum()) + 2, [f600],
                      [dict(passes=3, m=g12 + int(g3[:600].sum()) + 2, last_cell=int(order[600]), taken_last=4)]))
    cases.append(Case("heavy: 512 left, cut at its 3rd", order, g12m + int(g3m[:300].sum()) + 3, [fmix],
                      [dict(passes=3, m=g12m + int(g3m[:300].sum()) + 3, last_cell=int(order[300]), taken_last=5)]))
    # every candidate of a frame in ONE cell of the 1025-cell grid (all other cnt entries equal, e1 = e2 = 0 everywhere else): the
    # cell visited first (pass 2 never sees it: 1 + 3 features) and one visited in the second chunk (1 + 1 + 3)
    for k, most in ((0, 4), (1024, 5)):
        m = np.zeros(nc, int); j = np.zeros(nc, int); m[k], j[k] = 320, 180
        one = hand_table(rng, order, m, j, "random")
        for budget in (1, 3, most, most + 5):
            ex = dict(passes=1 if budget == 1 else 3, m=budget, last_cell=int(order[k]), taken_last=budget) if budget <= most else dict(passes=3, m=most)
            cases.append(Case("one cell (visited %d) budget %d" % (k, budget), order, budget, [one], [ex]))
    return cases


@cached
def sort_cases():
    """the stable sort of a cell (hso_select.hip:140-149: quality descending, ties in projection order) on cells of up to nine
    candidates with deleted (flags 2) and matched-and-deleted (flags 3) ones scattered through them (hand_table's junk): a budget
    nothing meets examines every candidate of the grid, so the whole order of every cell is compared; a second budget is cut in pass 3"""
    nc, cases = 1025, []
    order = order_for(nc)
    for qmode, seed in (("equal", 1), ("increasing", 2), ("two", 3), ("random", 4)):
        rng = np.random.default_rng(900 + seed)
        matched, junk = rng.integers(0, 5, nc), rng.integers(0, 5, nc)      # at most two successes left for pass 3: it walks every cell to its end
        matched[0] = min(matched[0], 3)
        frame = hand_table(rng, order, matched, junk, qmode)
        assert {0, 1, 2, 3} <= set(frame[2].tolist())
        g1, g2, g3 = pass_gains(matched)
        total = int(g1.sum() + g2.sum() + g3.sum())
        assert len(frame[0]) >= total + 55
        cases.append(Case("sort %s, everything examined" % qmode, order, total + 5, [frame], [dict(passes=3, m=total, n_examined=len(frame[0]))]))
        cases.append(Case("sort %s, cut in pass 3" % qmode, order, total - int(g3[700:].sum()) - 1, [frame]))
    return cases


def all_frame(rng, n, budget, at):
    """reprojectCellAll on n candidates: the budget-th match sits at index `at` (None: one match short of the budget)"""
    flags = rng.choice(JUNK, n)
    if at is None:
        flags[rng.choice(n, budget - 1, replace=False)] = 1
    else:
        flags[at] = 1
        flags[rng.choice(at, budget - 1, replace=False)] = 1
        flags[at + 1:] = rng.choice(np.array([0, 1, 2, 3], np.uint8), n - at - 1)       # never reached
    return rng.integers(0, 7, n).astype(np.int32), rng.integers(16, 80, n).astype(np.uint8), flags.astype(np.uint8)


@cached
def all_cases():
    """reprojectCellAll (hso_select.hip:106-113) with more than 1024 candidates: the scan of :78-89 over candidates, the emit loop
    of :111.  The completing candidate at the last index of a chunk, the first of the next, the very last, and nowhere.  (A budget of
    2000 or 4096 cannot be met before index budget - 1: there the first possible index stands for 1023.)"""
    cases, order = [], order_for(7)
    for budget, n, ats in ((1000, 1049, (CHUNK - 1, CHUNK, 1048, None)), (2000, 2049, (1999, 2 * CHUNK - 1, 2 * CHUNK, None)),
                           (4096, 4145, (4095, 4 * CHUNK, 4144, None))):
        rng = np.random.default_rng(budget)
        frames = [all_frame(rng, n, budget, at) for at in ats]
        expect = [dict(passes=0, m=budget - (at is None), n_examined=n if at is None else at + 1) for at in ats]
        frames.append(make_frame(rng, n, 7, 0.9, 0.03, False)); expect.append(None)
        cases.append(Case("all: %d of %d" % (budget, n), order, budget, frames, expect))
    return cases


@cached
def branch_cases():
    """n == max_fts + 49 takes reprojectCellAll, the same candidates plus one take the cells (hso_select.hip:106: n < budget + 50)"""
    cases, nc = [], 1025
    order = order_for(nc)
    for budget in (1, 200, 1000, 2000):
        rng = np.random.default_rng(40 + budget)
        more = make_frame(rng, budget + 50, nc, 0.9, 0.03, False)
        less = tuple(a[:-1] for a in more)
        cases.append(Case("branch switch at budget %d" % budget, order, budget, [less, more],
                          [dict(passes=0, branch=0), dict(branch=1)]))
    return cases


@cached
def small_cases():
    cases = []
    for nc in (1, 2, 1025, 2049):
        order = order_for(nc)
        rng = np.random.default_rng(60 + nc)
        frames = [make_frame(rng, 50, nc, 0.5, 0.1, False),             # max_fts = 1: 50 candidates -> reprojectCellAll, 51 -> the cells
                  make_frame(rng, 51, nc, 0.5, 0.1, False),
                  make_frame(rng, 51, nc, 0.0, 0.2, False),             # the cells, nothing matches: three passes for a budget of one
                  make_frame(rng, 3 * nc + 60, nc, 0.6, 0.1, False)]
        cases.append(Case("budget 1 on %d cells" % nc, order, 1, frames,
                          [dict(passes=0, branch=0), dict(branch=1), dict(passes=3, m=0, n_examined=51, branch=1), dict(branch=1)]))
        zero = dict(passes=0, m=0, n_examined=0, branch=0)
        cases.append(Case("budget 0 on %d cells" % nc, order, 0, frames + [EMPTY], [zero] * 5))   # hso_select.hip:104
    # nothing matched on 2049 cells (:184, :208 both taken with n_match == 0; every e1 without bit 30): every candidate examined
    nc = 2049
    rng = np.random.default_rng(61)
    frames = [make_frame(rng, 3000, nc, 0.0, 0.3, False), make_frame(rng, 5000, nc, 0.0, 0.0, True)]
    frames[0][2][::7] = 3                                                # matched and deleted among them
    cases.append(Case("nothing matched on 2049 cells", order_for(nc), 500, frames,
                      [dict(passes=3, m=0, n_examined=3000, branch=1), dict(passes=3, m=0, n_examined=5000, branch=1)]))
    return cases


GROUPS = dict(grids=grid_cases, cuts=cut_cases, heavy=heavy_cases, sort=sort_cases, all=all_cases, branch=branch_cases, small=small_cases)


# ------------------------------------------------------------------------------------------------------------------ CPU half
def check_aim(case):
    for k, ex in enumerate(case.expect):
        if ex is None:
            continue
        cell = case.frames[k][0]
        ref, m, passes = case.refs()[k]
        where = (case.name, k)
        if "passes" in ex:
            assert passes == ex["passes"], where
        if "m" in ex:
            assert m == ex["m"], where
        if "n_examined" in ex:
            assert len(ref) == ex["n_examined"], where
        if "branch" in ex:
            assert case.branch(k) == ex["branch"], where
        if "last_cell" in ex:                                            # the walk stopped at a feature of the cell the cut was aimed at
            assert ref[-1][1] and cell[ref[-1][0]] == ex["last_cell"] and m == case.budget, where
            assert sum(1 for i, t in ref if t and cell[i] == ex["last_cell"]) == ex["taken_last"], where


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_tables_aim_where_they_say(group):
    """the sequential walk alone: every hand-built table ends in the pass, on the branch, at the cell and with the number of features
    it was built for, and the ranges of a call start at offsets that are no multiple of 64"""
    for case in GROUPS[group]():
        check_aim(case)
        fb = case.begins()
        assert all(fb[k] % 64 != 0 for k in range(len(case.frames)) if len(case.frames[k][0]) and k > 0), case.name


def test_every_ending_occurs_at_every_chunked_grid():
    """random tables end in pass 1 or pass 3 only; with the constructed two-per-cell frame every grid of 1023 cells and more sees
    all four endings, and reprojectCellAll in the same calls"""
    seen = {nc: set() for nc in GRIDS}
    for case in grid_cases():
        for k in range(len(case.frames)):
            seen[len(case.order)].add(ending(case, k))
    for nc in GRIDS:
        if nc >= 1023:
            assert seen[nc] >= {"all", "pass 1", "passes 1 + 2", "pass 3", "pass 3 ran out"}, (nc, seen[nc])
        assert "?" not in seen[nc]


def test_heavy_cells_reach_the_packing_limits():
    """the cells the heavy tables are about, on the sequential walk: 598 taken-or-left successes behind passes 1 and 2 in the
    600-candidate cell (three of them taken when nothing cuts), a multiple of 256 left in the 514-matched cell"""
    case = heavy_cases()[0]
    cell, _, flags = case.frames[1]
    c = case.order[600]
    assert (cell == c).sum() == 600 and (flags[cell == c] == 1).all()
    ref, m, passes = case.refs()[1]
    assert passes == 3 and sum(1 for i, t in ref if t and cell[i] == c) == 5 and sum(1 for i, t in ref if cell[i] == c) == 5
    case = heavy_cases()[1]
    cell, _, flags = case.frames[1]
    for k, left in ((300, 512), (1023, 256), (1024, 257), (40, 258)):
        c = case.order[k]
        assert (flags[cell == c] == 1).sum() - 2 == left
        assert sum(1 for i, t in case.refs()[1][0] if t and cell[i] == c) == 5
    c = case.order[5]
    assert (cell == c).sum() == 300 and sum(1 for i, t in case.refs()[1][0] if cell[i] == c) == 300


# ------------------------------------------------------------------------------------------------------------------ GPU half
def run_on_device(ctx, case):
    fb = case.begins()
    cat = lambda j: np.concatenate([f[j] for f in case.frames])
    got, counts = ctx.reproject_select(fb, cat(0), cat(1), cat(2), case.order, case.budget)
    for k, (ref, m, passes) in enumerate(case.refs()):
        where = (case.name, "frame", k, "of", len(case.frames[k][0]), "candidates")
        assert tuple(int(v) for v in counts[k]) == (len(ref), m, passes, case.branch(k)), where
        g, r = np.array(got[k], np.int64).reshape(-1, 2), np.array(ref, np.int64).reshape(-1, 2)
        if not np.array_equal(g, r):
            at = int(np.argmax((g != r).any(axis=1)))
            assert False, where + ("first difference at", at, "device", tuple(g[at]), "walk", tuple(r[at]))


@pytest.mark.gpu
@pytest.mark.parametrize("n_cells", GRIDS)
def test_select_on_grids_around_the_chunk_size(gpu_ctx, n_cells):
    for case in grid_cases():
        if len(case.order) == n_cells:
            run_on_device(gpu_ctx, case)


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(set(GROUPS) - {"grids"}))
def test_select_on_hand_built_tables(gpu_ctx, group):
    for case in GROUPS[group]():
        run_on_device(gpu_ctx, case)
