"""Directed streams for the device emission chain (pure numpy, no GPU, no
engine import).

Every builder returns a case: the push cuts `(ts, kid, val)`, the window
parameters, the filter, and `facts` — what the case is ABOUT, computed from
the data by `simulate` (never restated as constants): per closing window the
touched and passing group counts, the row span (rows_seen at close minus
rows_seen at open), the key bit-length the engine derives from it, the
largest rebased first-seen key that actually passes, and per trigger the
route the engine must take, how the closes split into chains, each group
chain's `cshift` and each per-close chain's emission stream.

tests/test_emitvec_cpu.py pins these facts against the C oracle, so a case
that claims "4097 passers, 13-bit span" is known to be that before
tests/test_emission_edges_gpu.py runs it on the device.

The constants below restate the engine's (window_op.cpp / kernels.hip); the
route model is the documented one: above 65,536 live keys a trigger goes
through ONE group-batched chain per <= min(16, E_GELEMS / kcap) closes when
the passer hint (the passing count of the last close built) is at most
65,536, else through one per-close chain per close, close i of a chain group
on emission stream i % 4. A builder must leave the hint unambiguous: every
close of the preceding trigger on the same side of the threshold.
"""
from types import SimpleNamespace

import numpy as np

DEV_KEYS = 65_536       # device chains run above this many live keys
GROUP_HINT_MAX = 65_536  # passer hint at or below: group-batched chain
EGROUP = 16             # closes per chain group (E_POOL / 2)
E_GELEMS = 8 << 20      # group chain element capacity
NB = 512                # kcap granularity
RDIG = 11               # radix digit bits
RCHUNK = 4096           # elements per radix block
RSEG = 16               # segments of the parallel scan
CSTREAMS = 4            # emission streams (per-close chain round-robin)
VIEW_ROWS = 16_384      # slices at or above are served as views

SENTINEL = 69_999       # first row's id: n_keys > DEV_KEYS from row 0
NK = SENTINEL + 1
T0 = 1_000_000
LEN = 1000
FILTER = ("count", ">=", 2.0)
BIG = 70_000            # passers of a priming close (> GROUP_HINT_MAX)


def bitlen(x):
    return int(x).bit_length()


def radix_passes(bound):
    """launch_emission_sort's pass count for a host-known key bound."""
    p = max(2, -(-bitlen(bound) // RDIG))
    return p + (p & 1)


def kcap_of(n_keys):
    return -(-max(n_keys, NB) // NB) * NB


def scan_bs(n_keys):
    """blocks per scan segment of the per-close chain's radix grid"""
    return -(-(-(-n_keys // RCHUNK)) // RSEG)


def _snap(ts, len_ms):
    secs = len_ms // 1000
    if secs == 0:
        return ts - ts % len_ms
    return (ts // 1000 // secs) * secs * 1000


def windows_for_range(mn, mx, len_ms, slide_ms):
    """The frames one batch opens (get_windows_for_watermark restated)."""
    out = []
    if slide_ms:
        cur = _snap(mn - len_ms, len_ms)
        while cur <= mx:
            if not (mn > cur + len_ms or mx < cur):
                out.append((cur, cur + len_ms))
            cur += slide_ms
    else:
        cur = _snap(mn, len_ms)
        while cur <= mx:
            out.append((cur, cur + len_ms))
            cur += len_ms
    return out


def simulate(pushes, len_ms, slide_ms, filt, n_keys_hint):
    """Replay the pushes through the window/watermark/route model."""
    assert filt is None or filt == FILTER
    open_ = {}  # start -> frame
    rows_seen = 0
    wm = None
    n_keys = 0
    hint = (0, 0)  # (lowest, highest) passing count of the last trigger
    closes, triggers, open_after = [], [], []
    kcap = kcap_of(n_keys_hint)

    def trigger(push_idx):
        nonlocal hint
        due = [s for s in sorted(open_) if wm >= open_[s].end]
        if not due:
            return
        first = len(closes)
        for s in due:
            f = open_.pop(s)
            kid = np.concatenate(f.kid) if f.kid else np.zeros(0, np.int64)
            off = np.concatenate(f.off) if f.off else np.zeros(0, np.int64)
            uniq, idx, cnt = np.unique(kid, return_index=True,
                                       return_counts=True)
            ok = cnt >= 2 if filt else np.ones(len(uniq), bool)
            span = rows_seen - f.base
            closes.append(SimpleNamespace(
                start=s, end=f.end, touched=len(uniq), passing=int(ok.sum()),
                span=span, bits=bitlen(span),
                max_key=int((off[idx][ok] - f.base).max()) if ok.any() else -1,
                open_push=f.open_push, close_push=push_idx,
                trigger=len(triggers), route=None, chain=None, pos=None,
                stream=None))
        mine = closes[first:]
        assert kcap_of(max(n_keys, n_keys_hint)) == kcap, "state regrow"
        if n_keys <= DEV_KEYS:
            route, step = "host", EGROUP
        elif hint[1] <= GROUP_HINT_MAX:
            route, step = "group", min(EGROUP, max(1, E_GELEMS // kcap))
        elif hint[0] > GROUP_HINT_MAX:
            route, step = "perclose", EGROUP
        else:
            raise AssertionError("ambiguous passer hint %r" % (hint,))
        chains = []
        for g0 in range(0, len(mine), step):
            grp = mine[g0:g0 + step]
            cshift = bitlen(max(1, max(c.span for c in grp)))
            chains.append(SimpleNamespace(
                closes=list(range(first + g0, first + g0 + len(grp))),
                cshift=cshift, max_first=max(c.span for c in grp),
                passes=radix_passes(len(grp) << cshift
                                    | max(1, max(c.span for c in grp)))))
            for i, c in enumerate(grp):
                c.route, c.chain, c.pos = route, len(chains) - 1, i
                if route == "perclose":
                    c.stream = i % CSTREAMS
        triggers.append(SimpleNamespace(push=push_idx, route=route,
                                        chains=chains,
                                        closes=list(range(first, len(closes)))))
        hint = (min(c.passing for c in mine), max(c.passing for c in mine))

    for p, (ts, kid, _val) in enumerate(pushes):
        mn, mx = int(ts.min()), int(ts.max())
        n_keys = max(n_keys, int(kid.max()) + 1)
        for s, e in windows_for_range(mn, mx, len_ms, slide_ms):
            if s not in open_:
                open_[s] = SimpleNamespace(end=e, base=rows_seen, kid=[],
                                           off=[], open_push=p)
        for s, f in open_.items():
            m = np.flatnonzero((ts >= s) & (ts < f.end))
            if len(m):
                f.kid.append(kid[m])
                f.off.append(m + rows_seen)
        rows_seen += len(ts)
        if wm is None or wm <= mn:
            wm = mn
        trigger(p)
        open_after.append(len(open_))
    if open_:
        wm = max(wm, max(f.end for f in open_.values()))
        trigger(len(pushes))

    grp = [ch for t in triggers if t.route == "group" for ch in t.chains]
    return SimpleNamespace(
        closes=closes, triggers=triggers, open_after=open_after,
        n_keys=n_keys, kcap=kcap, rows=rows_seen,
        n_group_chains=len(grp),
        n_group_closes=sum(len(ch.closes) for ch in grp),
        group_max=max([len(ch.closes) for ch in grp] or [0]),
        n_perclose=sum(c.route == "perclose" for c in closes))


class _Stream:
    """Pushes under construction; values are drawn once, at the end."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.perm = self.rng.permutation(SENTINEL)  # ids below the sentinel
        self.pushes = []
        self.win = 0  # next tumbling window index

    def window(self, pairs, singles=0, lead=None):
        """Rows of the next 1 s tumbling window: `pairs` keys with two
        ADJACENT rows (they pass count >= 2) after `singles` keys with one
        row (touched, not passing); keys in shuffled order, so first-seen
        order is not id order. `lead` prepends given ids (one row each)."""
        ws = T0 + self.win * LEN
        self.win += 1
        if pairs + singles == BIG:  # every id, the sentinel's included
            keys = self.rng.permutation(NK)
        else:
            keys = self.perm[self.rng.permutation(pairs + singles)]
        kid = np.concatenate([
            np.asarray([] if lead is None else lead, np.int64),
            keys[:singles], np.repeat(keys[singles:], 2)]).astype(np.int64)
        n = len(kid)
        ts = ws + np.arange(n, dtype=np.int64) * LEN // max(n, 1)
        return ts, kid

    def gap(self):
        """skip one window: the next batch opens it with no rows"""
        self.win += 1

    def push(self, *chunks):
        self.pushes.append((np.concatenate([c[0] for c in chunks]),
                            np.concatenate([c[1] for c in chunks])))

    def tick(self):
        """a one-row batch in a window of its own: closes all before it"""
        self.push(self.window(0, 1))

    def case(self, name, n_keys_hint=NK, len_ms=LEN, slide_ms=0,
             filt=FILTER):
        pushes = [(ts, kid, self.rng.uniform(0, 115, len(ts)))
                  for ts, kid in self.pushes]
        for p in pushes:
            for a in p:
                a.setflags(write=False)
        assert pushes[0][1][0] >= SENTINEL, "sentinel row comes first"
        return SimpleNamespace(
            name=name, pushes=pushes, len_ms=len_ms, slide_ms=slide_ms,
            filt=filt, n_keys_hint=n_keys_hint,
            facts=simulate(pushes, len_ms, slide_ms, filt, n_keys_hint))


def count_pairs():
    """(touched, passing) of the per-close count-boundary closes, in trigger
    order: descending down each emission stream (position % 4), so a larger
    close precedes every smaller one on the same radix scratch."""
    t = scan_bs(NK) * RCHUNK  # first count that straddles a scan segment
    return [(t + 1, t + 1), (t, t), (t - 1, t - 1), (8192, 4096),
            (4097, 4097), (4096, 4096), (4095, 4095), (4097, 1),
            (1, 1), (1, 0)]


def perclose_counts(pairs=None, seed=4101):
    """Per-close chain at the live-count boundaries. A cold big close (group
    chain) arms the hint; four big closes then run per-close, one on each
    emission stream, and fill every histogram row of its radix scratch; the
    boundary closes follow in ONE trigger (plus a window with no rows:
    touched 0), so each reads scratch left by a larger close."""
    pairs = count_pairs() if pairs is None else pairs
    s = _Stream(seed)
    s.push(s.window(BIG - 1, 0, lead=[SENTINEL]))
    s.push(*[s.window(BIG) for _ in range(CSTREAMS)])      # closes the first
    chunks = [s.window(p, t - p) for t, p in pairs]
    s.gap()
    s.push(*chunks, s.window(3, 2))                        # closes the four
    s.tick()                                               # closes the cases
    return s.case("perclose_counts")


SPANS = (2 ** RDIG - 1, 2 ** RDIG, 2 ** RDIG + 1, 2 ** RDIG + 3)


def perclose_spans(spans=SPANS, seed=4202):
    """Per-close chain at the key-width boundary: windows whose row span is
    2^11 - 1, 2^11, 2^11 + 1 (two passes, second digit empty: the largest
    passing key is span - 3) and 2^11 + 3 (first span whose largest passing
    key, 2^11, uses the second digit). Each is primed by a big close and
    closed by a one-row batch: span = rows + 1."""
    s = _Stream(seed)
    lead = [SENTINEL]
    for sp in spans:
        s.push(s.window(BIG - len(lead), 0, lead=lead))
        lead = []
        rows = sp - 1
        s.push(s.window(rows // 2, rows % 2))
        s.tick()
    return s.case("perclose_spans")


BIG_ROWS = (1 << 22) + 100_002
EARLY, LATE = 4195, 100


def _big_window(s, lead=()):
    """~4.3M rows of one window over 4195 early groups (first seen at offset
    1000 j) and 100 late groups whose first row lies past offset 2^22, at
    2^22 + 1000 j + 500: their low 22 bits fall between the early groups'
    offsets, so a sort that drops the digits above bit 22 interleaves them
    with the early groups instead of placing them last."""
    ws = T0 + s.win * LEN
    s.win += 1
    early = s.perm[:EARLY].astype(np.int64)
    late = s.perm[5000:5000 + LATE].astype(np.int64)
    o = np.arange(BIG_ROWS, dtype=np.int64)
    seen = np.minimum(o // 1000, EARLY - 1) + 1   # early groups open so far
    kid = early[((o * 2654435761) >> 7) % seen]
    j = np.arange(EARLY)
    kid[j * 1000] = early
    j = np.arange(LATE)
    kid[(1 << 22) + j * 1000 + 500] = late
    kid[(1 << 22) + j * 1000 + 501] = late
    kid = np.concatenate([np.asarray(lead, np.int64), kid])
    n = len(kid)
    return ws + np.arange(n, dtype=np.int64) * LEN // n, kid


def perclose_span22(seed=4303):
    """The one large case: a per-close window spanning just over 2^22 rows,
    where the pass count goes from 2 to 4."""
    s = _Stream(seed)
    s.push(s.window(BIG - 1, 0, lead=[SENTINEL]))
    s.push(_big_window(s))
    s.tick()
    return s.case("perclose_span22")


def group_span22(seed=4404):
    """Group chain whose FIRST close spans >= 2^22 rows beside two tiny
    ones: the long window stays open (one late row keeps the batch minimum
    inside it) while the next two open and fill; one batch closes all
    three, and max_first comes from the long close alone."""
    s = _Stream(seed)
    big = _big_window(s, lead=[SENTINEL])
    s.push(big)
    late_row = (big[0][-1:], big[1][-1:])
    s.push(late_row, s.window(300, 7), s.window(1, 1))
    s.tick()
    return s.case("group_span22")


def group_sizes(seed=4505):
    """Group chain: groups of exactly 1, 2 and 16 closes and a 17-close
    trigger (16 + 1); cshift 11 and 12 with two closes each (the close
    index lands on, and just past, a digit boundary); inside the 16: closes
    with no rows, no passer, one passer, every group passing, and slices on
    both sides of the view threshold."""
    s = _Stream(seed)
    # 2 closes, span 1024..2047: cshift 11
    s.push(s.window(300, 99, lead=[SENTINEL]), s.window(350, 100))
    s.tick()
    # 2 closes, span 2048..4095: cshift 12
    s.push(s.window(700, 50), s.window(600, 1))
    s.tick()
    shape16 = [(300, 0), (0, 200), (1, 150), (20_000, 0), (1, 0), (0, 1),
               (5000, 0), (VIEW_ROWS, 0), (VIEW_ROWS - 1, 0), (40, 40),
               (2048, 0), (0, 2047), (7, 3), (1, 1), (64, 0)]
    chunks = [s.window(p, q) for p, q in shape16[:8]]
    s.gap()  # the 16th close: a window no row falls in
    chunks += [s.window(p, q) for p, q in shape16[8:]]
    s.push(*chunks)
    s.tick()
    s.push(*[s.window(50 + i, i % 3) for i in range(17)])
    s.tick()
    return s.case("group_sizes")


CAP_KEYS = 600_000


def group_cap(seed=4606):
    """Group cap: ~600k keys make E_GELEMS / kcap = 13 < 16. One batch of a
    few hundred rows leaves 20 sliding windows open (1 s long, 100 ms hop),
    the next closes them in one trigger: chains of 13 + 7 closes."""
    s = _Stream(seed)
    n = 450
    keys = s.perm[:150].astype(np.int64)
    kid = np.concatenate([[CAP_KEYS - 1], keys[s.rng.integers(0, 150, n)]])
    # rows over [T0, T0 + 1050]: frames T0 - 1000 .. T0 + 1000; the first
    # ends AT the batch minimum, so it closes (empty) with this very batch
    ts = T0 + np.arange(n + 1, dtype=np.int64) * 1050 // n
    s.pushes.append((ts, kid.astype(np.int64)))
    s.pushes.append((np.array([T0 + 10_050], np.int64),
                     np.array([int(keys[0])], np.int64)))
    return s.case("group_cap", n_keys_hint=CAP_KEYS, slide_ms=100)


def small_counts(seed=4707):
    """The count cases the single-block sort is run on."""
    c = perclose_counts(pairs=[(4097, 4097), (1, 1)], seed=seed)
    c.name = "small_counts"
    return c


BUILDERS = {f.__name__: f for f in (
    perclose_counts, perclose_spans, perclose_span22, group_span22,
    group_sizes, group_cap, small_counts)}
