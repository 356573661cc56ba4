"""The layout part of datok_amd/csrc/dtk_mirror.h without a GPU: a small program of its own (address and undefined-
behaviour sanitizers on) describes the tables that are built on it -- a slice's offsets in both forms, its sentence rows,
the batch's sentence table -- and prints where the pieces lie and which byte ranges the first copies and the late
requests ask for.  The test checks them against the rules stated here, in Python: pieces on multiples of 8, one home count
per piece, ranges that join only across a piece's end, and the number of first copies a slice enqueues.  The same program
drives the plain-data part of a derived table's protocol (DerivedState, DerivedReads, derived_complete) and prints what it
did: the lines tagged X."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "datok_amd", "csrc")
TOKENS = (0, 1, 63, 64, 65)
CAPS = (0, 1, 7)
HOMES = (0, 1, -1)          # -1: the capacity

_CPP = r'''
#define DTK_MIRROR_LAYOUT_ONLY
#include "dtk_mirror.h"
#include <cstdio>
struct OffsTrailer { uint64_t w[9]; };             // (stand-ins of the trailers' and the head's sizes)
struct SensTrailer { uint64_t w[14]; };
struct Head64 { int64_t base0, base1; uint32_t brk, reserved; };
typedef unsigned long long ull;

static void ranges(const char *tag, MirrorLayout &L) {   // prints the pending ranges and takes them, as a copy would
  std::printf("%s", tag);
  for (const MirrorLayout::Range &r : L.pending) std::printf(" %llu:%llu", (ull)r.from, (ull)r.to);
  std::printf("\n");
  L.pending.clear();
}
static void pieces(const MirrorLayout &L) {
  for (const MirrorLayout::Part &q : L.parts) std::printf("P %llu %llu %llu %llu\n", (ull)q.at, (ull)q.size, (ull)q.cap, (ull)q.home);
  std::printf("B %llu\n", (ull)L.bytes);
}
template <class T> void late(MirrorLayout &L, Piece<T> p) {   // two more elements than are home, twice
  const uint64_t n = L.home(p) + 2;
  std::printf("N %u %llu\n", p.i, (ull)n);
  L.bring(p, n); ranges("L", L);
  L.bring(p, n); ranges("L", L);
  std::vector<uint64_t> block(L.bytes / 8 + 1);
  T *q = L.in(block.data(), p);                                 // the typed pointer into a block: at the piece's offset
  std::printf("H %llu %d\n", (ull)L.home(p), (int)((uint8_t *)q == (uint8_t *)block.data() + L.at(p)));
}
template <class... P> void late_all(MirrorLayout &L, P... p) { (late(L, p), ...); }

// A stage as dtk_derived.cpp drives one: step() launches where nothing is built, into a block of max(need, bound)
// elements; the count word then reads counts[launch - 1].
namespace { struct Stage { DerivedState s; int launches = 0; uint64_t cap = 0; }; }
static void complete(const char *tag, Stage &g, uint64_t bound, std::vector<uint64_t> counts, int step_rc = 0) {
  int reads = 0;
  const int rc = derived_complete(
      g.s, [&] { if (!g.s.built) { g.cap = std::max(g.s.need, bound); g.s.launched(); g.launches++; } return step_rc; },
      [&](uint64_t &n) { reads++; n = counts[g.launches - 1]; return n <= g.cap; });
  std::printf("X %s %d %d %d %d %llu %llu %u\n", tag, rc, g.launches, reads, (int)g.s.built, (ull)g.s.need, (ull)g.cap, g.s.gen);
}
static void protocol() {
  { Stage g; complete("fits", g, 4, {3}); complete("fits_again", g, 4, {3}); }
  { Stage g; complete("overflow", g, 4, {10, 10}); }
  { Stage g; complete("overflow_twice", g, 4, {10, 20}); }
  { Stage g; complete("step_fails", g, 4, {3}, -5); }
  for (int keep = 0; keep < 2; keep++) {   // a new run: the need resets, or (the pieces) survives
    Stage g; complete(keep ? "run1_keep" : "run1_reset", g, 4, {10, 10});
    g.s.new_run(keep != 0);
    std::printf("X %s %d %llu %u\n", keep ? "new_run_keep" : "new_run_reset", (int)g.s.built, (ull)g.s.need, g.s.gen);
    g.launches = 0; complete(keep ? "run2_keep" : "run2_reset", g, 4, {10, 10});
  }
  const DerivedReads r{3, 7};                // what a consumer recorded: (g_wp, g_sen)
  std::printf("X stale %d %d %d %d\n", (int)r.stale(3, 7), (int)r.stale(4, 7), (int)r.stale(3, 8), (int)r.stale(4, 8));
  // the batch's sentence table as sen_enqueue asks for it: the pieces in the block's order, the count word last
  for (int mode = 0; mode < 3; mode++) {     // 0: whole block at build; 1: count only; 2: count at build, the block later
    MirrorLayout L;
    Piece<uint64_t> off; Piece<uint32_t> tok_end, bstart, bend; Piece<int32_t> rs, re; Piece<uint32_t> tse, cnt;
    L.add(off, 4); L.add(tok_end, 5); L.add(bstart, 5); L.add(bend, 5); L.add(rs, 5); L.add(re, 5); L.add(tse, 3); L.add(cnt, 1);
    auto block = [&] { L.bring(off, 4); L.bring(tok_end, 5); L.bring(bstart, 5); L.bring(bend, 5); L.bring(rs, 5); L.bring(re, 5); L.bring(tse, 3); };
    if (mode == 0) block();
    L.bring(cnt, 1);
    std::printf("X sen%d %llu %llu", mode, (ull)L.at(cnt), (ull)L.bytes);
    ranges("", L);
    if (mode == 2) { block(); L.bring(cnt, 1); std::printf("X sen2_later %llu %llu", (ull)L.at(tse), (ull)L.at(cnt)); ranges("", L); }
    if (mode == 1) {                         // the host wrote the whole copy itself (the splice): nothing is missing
      L.all_home(); block(); L.bring(cnt, 1);
      std::printf("X sen1_all_home %llu %llu", (ull)L.home(tok_end), (ull)L.home(cnt)); ranges("", L);
    }
  }
}

int main() {
  protocol();
  const uint64_t tokens[] = {0, 1, 63, 64, 65}, caps[] = {0, 1, 7};
  const int homes[] = {0, 1, -1};
  for (uint64_t nt : tokens) for (uint64_t cap : caps) for (int hm : homes) {
    const uint64_t home = hm < 0 ? cap : (uint64_t)hm;
    for (int blocked = 0; blocked < 2; blocked++) {
      MirrorLayout L;
      Piece<int64_t> rstart, rend, sent; Piece<OffsTrailer> trailer; Piece<uint32_t> ttok, tsent; Piece<Head64> heads; Piece<uint32_t> words;
      L.add(rstart, nt); L.add(rend, nt); L.add(sent, cap); L.add(trailer, 1); L.add(ttok, cap); L.add(tsent, cap);
      L.add(heads, blocked ? (nt + 63) / 64 : 0); L.add(words, blocked ? nt : 0);
      std::printf("case %s %llu %llu %llu\n", blocked ? "offs_blocked" : "offs_plain", (ull)nt, (ull)cap, (ull)home);
      if (!blocked) { L.bring(rstart, nt); L.bring(rend, nt); }
      L.bring(sent, home); L.bring(trailer, 1); L.bring(ttok, home); L.bring(tsent, home);
      L.bring(heads, L.cap(heads)); L.bring(words, L.cap(words));
      ranges("R", L); pieces(L);
      if (blocked) { L.bring(rstart, nt); L.bring(rend, nt); ranges("F", L); }   // (blk_fail: the plain pair comes late)
      late_all(L, rstart, rend, sent, trailer, ttok, tsent, heads, words);
    }
    {
      MirrorLayout L;
      Piece<SensTrailer> trailer; Piece<uint32_t> tse, tok_end; Piece<uint64_t> bstart, bend; Piece<int64_t> rs, re;
      L.add(trailer, 1); L.add(tse, cap); L.add(tok_end, cap); L.add(bstart, cap); L.add(bend, cap); L.add(rs, cap); L.add(re, cap);
      std::printf("case sens %llu %llu %llu\n", (ull)nt, (ull)cap, (ull)home);
      L.bring(trailer, 1); L.bring(tse, home);
      L.bring(tok_end, home); L.bring(bstart, home); L.bring(bend, home); L.bring(rs, home); L.bring(re, home);
      ranges("R", L); pieces(L);
      late_all(L, trailer, tse, tok_end, bstart, bend, rs, re);
    }
    for (uint64_t docs = 1; docs <= 3; docs += 2) {
      MirrorLayout L;
      Piece<uint64_t> off; Piece<uint32_t> tok_end, bstart, bend; Piece<int32_t> rs, re; Piece<uint32_t> tse, cnt;
      L.add(off, docs + 1); L.add(tok_end, cap); L.add(bstart, cap); L.add(bend, cap); L.add(rs, cap); L.add(re, cap);
      L.add(tse, nt); L.add(cnt, 1);
      std::printf("case sen%llu %llu %llu %llu\n", (ull)docs, (ull)nt, (ull)cap, (ull)cap);
      L.bring(off, docs + 1); L.bring(tok_end, cap); L.bring(bstart, cap); L.bring(bend, cap); L.bring(rs, cap); L.bring(re, cap);
      L.bring(tse, nt); L.bring(cnt, 1);
      ranges("R", L); pieces(L);
      late_all(L, off, tok_end, bstart, bend, rs, re, tse, cnt);
      L.clear();
      std::printf("C %llu %llu %llu\n", (ull)L.bytes, (ull)L.parts.size(), (ull)L.pending.size());
    }
  }
  return 0;
}
'''


def _sizes(table):
    """Element sizes of the table's pieces, in the order they are added."""
    return {"offs_plain": (8, 8, 8, 72, 4, 4, 24, 4), "offs_blocked": (8, 8, 8, 72, 4, 4, 24, 4),
            "sens": (112, 4, 4, 8, 8, 8, 8), "sen1": (8, 4, 4, 4, 4, 4, 4, 4), "sen3": (8, 4, 4, 4, 4, 4, 4, 4)}[table]


def _caps(table, nt, cap):
    if table.startswith("offs"):
        blocked = table == "offs_blocked"
        return (nt, nt, cap, 1, cap, cap, (nt + 63) // 64 if blocked else 0, nt if blocked else 0)
    if table == "sens":
        return (1, cap, cap, cap, cap, cap, cap)
    return (int(table[3:]) + 1, cap, cap, cap, cap, cap, nt, 1)


def _first(table, nt, cap, home):
    """The first pass's requests, (piece, elements) in order."""
    if table.startswith("offs"):
        plain = [(0, nt), (1, nt)] if table == "offs_plain" else []
        return plain + [(2, home), (3, 1), (4, home), (5, home), (6, 1 << 62), (7, 1 << 62)]
    if table == "sens":
        return [(0, 1)] + [(i, home) for i in range(1, 7)]
    return [(i, 1 << 62) for i in range(8)]


def _pad8(x):
    return (x + 7) // 8 * 8


def _expect(sizes, caps, at, homes, requests):
    """The merge rule, restated: a request yields the bytes of the elements [home, min(n, cap)); it goes into the range in
    front of it only if that range ended its own piece, this one begins its piece, and nothing but padding lies between."""
    out, last = [], None                                   # last: the piece the last range ended, if it ended it
    for i, n in requests:
        n = min(n, caps[i])
        if n <= homes[i]:
            continue
        lo, hi = at[i] + homes[i] * sizes[i], at[i] + n * sizes[i]
        if out and (lo == out[-1][1] or (last is not None and homes[i] == 0 and at[i] == _pad8(out[-1][1])
                                         and all(caps[j] == 0 for j in range(last + 1, i)) and i > last)):
            out[-1][1] = hi
        else:
            out.append([lo, hi])
        last = i if n == caps[i] else None
        homes[i] = n
    return [tuple(r) for r in out]


def _parse(lines):
    cases, cur = [], None
    for l in lines:
        tag, *f = l.split()
        if tag == "case":
            cur = dict(table=f[0], nt=int(f[1]), cap=int(f[2]), home=int(f[3]), P=[], late=[], F=None, C=None)
            cases.append(cur)
        elif tag in ("R", "F"):
            cur[tag] = [tuple(int(x) for x in r.split(":")) for r in f]
        elif tag == "P":
            cur["P"].append(tuple(int(x) for x in f))
        elif tag == "B":
            cur["B"] = int(f[0])
        elif tag == "N":
            cur["late"].append(dict(i=int(f[0]), n=int(f[1]), L=[]))
        elif tag == "L":
            cur["late"][-1]["L"].append([tuple(int(x) for x in r.split(":")) for r in f])
        elif tag == "H":
            cur["late"][-1]["H"], cur["late"][-1]["ptr_ok"] = int(f[0]), int(f[1])
        elif tag == "C":
            cur["C"] = tuple(int(x) for x in f)
    return cases


_PROTOCOL = {}   # the X lines of the program's one run: tag -> fields


@pytest.fixture(scope="module")
def protocol(cases):
    return {k: [int(x) if ":" not in x else tuple(int(y) for y in x.split(":")) for x in v] for k, v in _PROTOCOL.items()}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("mirror")
    src, exe = d / "mirror_layout.cpp", d / "mirror_layout"
    src.write_text(_CPP)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0 and not out.stderr, out.stderr.decode()
    got = _parse(l for l in out.stdout.decode().splitlines() if not l.startswith("X "))
    _PROTOCOL.update({f[1]: f[2:] for f in (l.split() for l in out.stdout.decode().splitlines()) if f[0] == "X"})
    assert len(got) == len(TOKENS) * len(CAPS) * len(HOMES) * 5
    return got


def test_every_case_was_laid_out(cases):
    seen = {(c["table"], c["nt"], c["cap"], c["home"]) for c in cases}
    for t in ("offs_plain", "offs_blocked", "sens"):
        for nt in TOKENS:
            for cap in CAPS:
                for hm in HOMES:
                    assert (t, nt, cap, cap if hm < 0 else hm) in seen
    for t in ("sen1", "sen3"):
        assert {(nt, cap) for (tt, nt, cap, _) in seen if tt == t} == {(nt, cap) for nt in TOKENS for cap in CAPS}


def test_pieces_start_on_multiples_of_8_and_do_not_overlap(cases):
    for c in cases:
        sizes, caps = _sizes(c["table"]), _caps(c["table"], c["nt"], c["cap"])
        assert [(p[1], p[2]) for p in c["P"]] == list(zip(sizes, caps)), c     # the element type and capacity as added
        end = 0
        for at, size, cap, _ in c["P"]:
            assert at % 8 == 0 and at == end, c                                 # in order, no gap but the padding, no overlap
            end = _pad8(at + size * cap)
            assert end - (at + size * cap) < 8
            if cap == 0:
                assert end == at                                               # a piece of no element takes no room
        assert c["B"] == end, c                                                 # the total: the last piece's padded end


def test_first_copies_number_as_stated_and_cover_what_was_asked_for(cases):
    headline = {"offs_plain": 3, "offs_blocked": 4, "sens": 6, "sen1": 1, "sen3": 1}
    for c in cases:
        t, nt, cap = c["table"], c["nt"], c["cap"]
        sizes, caps, at = _sizes(t), _caps(t, nt, cap), [p[0] for p in c["P"]]
        homes = [0] * len(sizes)
        want = _expect(sizes, caps, at, homes, _first(t, nt, cap, c["home"]))
        assert c["R"] == want, c
        assert [p[3] for p in c["P"]] == homes, c                               # the one home count per piece
        # every byte asked for is in a range; a range holds nothing else but padding, and nothing outside the block
        asked = [(at[i], at[i] + homes[i] * sizes[i]) for i in range(len(sizes)) if homes[i]]
        pad = [(at[i] + sizes[i] * caps[i], _pad8(at[i] + sizes[i] * caps[i])) for i in range(len(sizes))]
        for lo, hi in asked:
            assert any(r[0] <= lo and hi <= r[1] for r in c["R"]), c
        covered = sum(r[1] - r[0] for r in c["R"])
        inside_pad = sum(min(hi, r[1]) - max(lo, r[0]) for lo, hi in pad for r in c["R"] if min(hi, r[1]) > max(lo, r[0]))
        assert covered == sum(hi - lo for lo, hi in asked) + inside_pad, c
        assert all(0 <= r[0] < r[1] <= c["B"] for r in c["R"]) and all(a[1] <= b[0] for a, b in zip(c["R"], c["R"][1:])), c
        # the counts of the first pass where no piece but the whole ones ends at its capacity: 3 (plain), 4 (blocked; 3 with
        # no token), 6 (rows), 1 (the batch's table, always)
        if t.startswith("sen") and t != "sens":
            assert len(c["R"]) == 1, c
        elif cap == 7 and c["home"] == 1:
            assert len(c["R"]) == (3 if t == "offs_blocked" and nt == 0 else headline[t]), c
        else:
            assert len(c["R"]) <= headline[t], c                                # fewer where a piece happens to be whole or empty
        if t == "offs_blocked":                                                # blk_fail: the plain pair, one range behind the rest
            assert c["F"] == ([(0, at[2])] if nt else []), c


def test_late_requests_bring_exactly_the_missing_elements_once(cases):
    for c in cases:
        sizes, caps = _sizes(c["table"]), _caps(c["table"], c["nt"], c["cap"])
        homes = [p[3] for p in c["P"]]
        if c["table"] == "offs_blocked":
            homes[0] = homes[1] = c["nt"]                                       # (the F requests brought the pair)
        assert [q["i"] for q in c["late"]] == list(range(len(sizes))), c
        for q in c["late"]:
            i, at = q["i"], c["P"][q["i"]][0]
            assert q["n"] == homes[i] + 2 and q["ptr_ok"] == 1, c
            n = min(q["n"], caps[i])                                            # clamped at the capacity
            first = [(at + homes[i] * sizes[i], at + n * sizes[i])] if n > homes[i] else []
            assert q["L"] == [first, []], (c, q)                                # ... and a second identical request: nothing
            assert q["H"] == max(n, homes[i]), (c, q)
            if caps[i] == 0:
                assert first == [] and q["H"] == 0, (c, q)                      # a piece of no element: nothing
        if c["C"] is not None:
            assert c["C"] == (0, 0, 0)                                          # clear(): a new description starts empty


E_STATE = -8   # DTK_E_STATE


def test_a_table_that_overflows_is_launched_exactly_once_more(protocol):
    # fields: rc, launches, count reads, built, need, capacity, gen
    assert protocol["fits"] == [0, 1, 1, 1, 0, 4, 1]
    assert protocol["fits_again"] == [0, 1, 1, 1, 0, 4, 1]               # complete already: no launch, this call reads the count once
    assert protocol["overflow"] == [0, 2, 2, 1, 10, 10, 2]               # need is the count, the second block holds it
    assert protocol["overflow_twice"] == [E_STATE, 2, 2, 1, 10, 10, 2]   # a run's count cannot grow: no third launch
    assert protocol["step_fails"] == [-5, 1, 0, 1, 0, 4, 1]              # the step's error comes out, no count is read


def test_a_new_run_clears_built_and_the_resetting_need_and_keeps_the_surviving_one(protocol):
    assert protocol["run1_reset"] == protocol["run1_keep"] == [0, 2, 2, 1, 10, 10, 2]
    assert protocol["new_run_reset"] == [0, 0, 2]                        # built, need, gen (launches are still counted)
    assert protocol["new_run_keep"] == [0, 10, 2]
    assert protocol["run2_reset"] == [0, 2, 2, 1, 10, 10, 4]             # the bound again, and the overflow again
    assert protocol["run2_keep"] == [0, 1, 1, 1, 10, 10, 3]              # the run starts with the block the last one needed


def test_a_consumer_is_stale_exactly_when_a_generation_it_read_has_moved(protocol):
    assert protocol["stale"] == [0, 1, 1, 1]


def test_sentence_table_bring_order_gives_one_range(protocol):
    at_cnt, size = protocol["sen0"][:2]
    assert size == at_cnt + 8
    assert protocol["sen0"][2:] == [(0, at_cnt + 4)]                     # the whole block at build: one copy, the count word its end
    assert protocol["sen1"][2:] == [(at_cnt, at_cnt + 4)]                # the count only: 4 bytes
    assert protocol["sen2"][2:] == [(at_cnt, at_cnt + 4)]
    at_tse, at_cnt2 = protocol["sen2_later"][:2]
    assert at_cnt2 == at_cnt and at_tse + 3 * 4 <= at_cnt
    assert protocol["sen2_later"][2:] == [(0, at_tse + 3 * 4)]           # the block later: one range that stops short of the count word
    assert protocol["sen1_all_home"] == [5, 1]                           # all_home(): every piece whole, and nothing more to ask for
