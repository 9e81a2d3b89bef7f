"""The ingest ring's accounting under overflow (csrc/fmd_ring.c: inflight, debt, take / release / un-take), without a device.

On a device these paths run only when a writer overflows a ring while a job's H2D copy is in flight, or when a launch fails after bytes were
taken.  tests/c/ring_check.c links fmd_ring.c alone - no ROCm header, no library: the unit is device-free - and is built here with
AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program.  Random command sequences are held against a model that
tracks ABSOLUTE stream positions: W bytes written so far, absR = the absolute position of the oldest byte still in the ring (W - size), and the
FIFO of at most two outstanding jobs (start, take), as the pump has them."""
import os
import random
import shutil
import subprocess
import tempfile
from collections import namedtuple

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl_fm_player_amd", "csrc")
DROP_OLDEST, REFERENCE = 0, 1
Counters = namedtuple("Counters", "rpos wpos size inflight debt dropped")


def lcg_bytes(n, seed):
    """The bytes `push n seed` of ring_check.c writes."""
    out, x = bytearray(), seed
    for _ in range(n):
        x = (1664525 * x + 1013904223) & 0xFFFFFFFF
        out.append(x >> 24)
    return bytes(out)


class RingCheck:
    """One ring_check process; cmd() sends a line and returns (Counters, the rest of the answer as words)."""

    def __init__(self, exe, err):
        self.err = err
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")     # (the leak checker needs ptrace, which not every sandbox grants)
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=err, text=True, bufsize=1, env=env)

    def cmd(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        w = self.p.stdout.readline().split()
        assert len(w) >= 6, "ring_check died at %r: %s" % (line, open(self.err.name).read()[-2000:])
        return Counters(*map(int, w[:6])), w[6:]

    def peek(self, frm, n):
        _, rest = self.cmd("peek %d %d" % (frm, n))
        return bytes.fromhex(rest[0]) if rest else b""

    def close(self):
        self.p.stdin.close()
        rc = self.p.wait(timeout=60)
        report = open(self.err.name).read()
        assert rc == 0 and not report, "ring_check exit %d: %s" % (rc, report[-2000:])     # (a sanitizer finding lands here)


@pytest.fixture(scope="module")
def ring_check():
    tmp = tempfile.mkdtemp(prefix="fmd_ring_")
    exe = os.path.join(tmp, "ring_check")
    subprocess.run(["cc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "c", "ring_check.c"), os.path.join(CSRC, "fmd_ring.c"), "-lpthread"], check=True)
    rings = []

    def start():
        rings.append(RingCheck(exe, open(os.path.join(tmp, "stderr_%d.txt" % len(rings)), "w+")))
        return rings[-1]
    yield start
    for r in rings:
        if r.p.poll() is None:
            r.p.kill()
        r.err.close()
    shutil.rmtree(tmp, ignore_errors=True)


class Model:
    """Drop-oldest mode in absolute positions.  Every step asserts the counters ring_check printed against it."""

    def __init__(self, ring, cap):
        self.ring, self.cap = ring, cap
        self.data = bytearray()          # every byte ever pushed: W = len(data)
        self.absR = 0
        self.jobs = []                   # (start, take), oldest first
        self.released = self.popped = 0
        self.c, _ = ring.cmd("new %d %d" % (cap, DROP_OLDEST))
        self.check()

    @property
    def W(self):
        return len(self.data)

    def check(self):
        c, cap = self.c, self.cap
        # 2: the counters are consistent, and the ring's window is the model's
        assert 0 <= c.inflight <= c.size <= cap and (c.rpos + c.size) % cap == c.wpos
        assert self.W - c.size == self.absR and c.rpos == self.absR % cap
        # 1: what the jobs hold is in flight or already released by an overflow
        assert c.inflight + c.debt == sum(t for _, t in self.jobs)
        if self.jobs:
            assert self.absR - c.debt >= self.jobs[0][0]        # (>: an overflow ate a whole job and more, and the next job started beyond it)
        else:
            assert c.debt == 0
        # 7: every byte pushed is in the ring, or was released, popped or dropped
        assert c.dropped == self.W - c.size - self.released - self.popped

    def push(self, n, seed):
        assert 1 <= n <= self.cap
        self.data += lcg_bytes(n, seed)
        self.absR = max(self.absR, self.W - self.cap)
        self.c, _ = self.ring.cmd("push %d %d" % (n, seed))
        self.check()
        assert self.ring.peek(self.c.rpos, self.c.size) == self.data[self.absR:]     # the ring holds the newest bytes, in order

    def ready(self):
        return self.c.size - self.c.inflight

    def take(self, t):
        """3: the job starts behind everything in flight, and its bytes are the stream's at that position."""
        assert 0 < t <= self.ready()
        start = self.absR + self.c.inflight
        self.c, (frm,) = self.ring.cmd("take %d" % t)
        assert int(frm) == start % self.cap
        self.jobs.append((start, t))
        self.check()
        assert self.ring.peek(int(frm), t) == self.data[start:start + t]
        return start

    def release(self):
        """4: the oldest job's bytes leave the ring - those an overflow has not released already."""
        s, t = self.jobs.pop(0)
        before = self.absR
        self.absR = max(before, s + t)
        self.released += self.absR - before
        self.c, _ = self.ring.cmd("release %d" % t)
        self.check()

    def untake(self):
        """5: the newest job goes back to `buffered`; the other job's share of the debt stays.  Returns (start, take) of the job undone."""
        s, t = self.jobs.pop()
        old = self.jobs[0][1] if self.jobs else 0
        was = self.c
        self.c, _ = self.ring.cmd("untake %d %d" % (t, old))
        assert (self.c.rpos, self.c.size, self.c.wpos, self.c.dropped) == (was.rpos, was.size, was.wpos, was.dropped)
        self.check()
        assert self.absR + self.c.inflight == max(s, self.absR)          # where the next job starts: the same place, unless an overflow moved past it
        return s, t

    def pop(self, n):
        """6: nothing while a job holds the bytes in front; else the oldest bytes in order."""
        want = b"" if (self.jobs or self.c.debt or self.c.size < n) else bytes(self.data[self.absR:self.absR + n])
        self.c, rest = self.ring.cmd("pop %d" % n)
        assert int(rest[0]) == len(want) and (bytes.fromhex(rest[1]) if len(rest) > 1 else b"") == want
        self.absR += len(want)
        self.popped += len(want)
        self.check()


@pytest.mark.parametrize("cap", [16, 24, 64])
def test_random_sequences_hold_the_invariants(ring_check, cap):
    ring = ring_check()
    seen = dict(debt=0, debt_two_jobs=0, untake_debt=0, untake_old_debt=0, retake=0, moved_past=0, pops=0, job_eaten_whole=0)
    for seed in range(200):
        rng = random.Random(1000 * cap + seed)
        bl = rng.choice([2, 4, 8])
        m = Model(ring, cap)
        for _ in range(60):
            op = rng.random()
            if op < 0.45:
                m.push(rng.randint(1, cap), rng.getrandbits(32))
            elif op < 0.70 and len(m.jobs) < 2:
                nb = min(m.ready() // bl, rng.randint(1, 4))           # a job is whole blocks that are ready
                if nb:
                    m.take(nb * bl)
            elif op < 0.85 and m.jobs:
                m.release()
            elif op < 0.93 and m.jobs:
                seen["untake_debt"] += m.c.debt > 0
                seen["untake_old_debt"] += m.c.debt > 0 and len(m.jobs) == 2
                s, t = m.untake()
                seen["moved_past"] += m.absR > s
                if m.ready() >= t and rng.random() < 0.5:
                    assert m.take(t) == max(s, m.absR)                     # (take() holds `from` and the bytes against this position)
                    seen["retake"] += 1
            else:
                m.pop(bl * rng.randint(1, 2))
                seen["pops"] += not m.jobs and m.c.debt == 0
            seen["debt"] += m.c.debt > 0
            seen["debt_two_jobs"] += m.c.debt > 0 and len(m.jobs) == 2
            seen["job_eaten_whole"] += bool(m.jobs) and m.absR >= sum(m.jobs[0])
    ring.close()
    assert all(seen.values()), seen                                       # the sequences did reach the paths this test is about


def test_push_longer_than_the_ring_keeps_the_newest_bytes(ring_check):
    ring = ring_check()
    c, _ = ring.cmd("new 16 %d" % DROP_OLDEST)
    c, _ = ring.cmd("push 5 1")
    c, _ = ring.cmd("push 40 2")
    assert (c.size, c.inflight, c.debt, c.dropped) == (16, 0, 0, (40 - 16) + 5) and (c.rpos + c.size) % 16 == c.wpos
    c, rest = ring.cmd("pop 16")
    assert rest[0] == "16" and bytes.fromhex(rest[1]) == lcg_bytes(40, 2)[-16:] and c.size == 0 and c.dropped == 29
    ring.close()


@pytest.mark.parametrize("second_push,debt_after_untake,absr_after_release", [
    (6, 2, 4),          # the overflow eats 2 bytes of the older job: un-taking the newer one leaves that debt for the older job's release
    (10, 4, 6),         # ... the whole older job and 2 bytes of the newer: only those 2 are the newer job's, and already released
])
def test_untake_leaves_the_older_jobs_share_of_the_debt(ring_check, second_push, debt_after_untake, absr_after_release):
    ring = ring_check()
    m = Model(ring, 16)
    m.push(12, 7)
    assert (m.take(4), m.take(4)) == (0, 4)                               # the older job holds [0, 4), the newer [4, 8)
    m.push(second_push, 8)
    over = 12 + second_push - 16
    assert (m.absR, m.c.debt, m.c.inflight) == (over, over, 8 - over)
    m.untake()                                                            # old = the older job's take, 4
    assert (m.c.debt, m.c.inflight, m.absR) == (debt_after_untake, 4 - debt_after_untake, over)
    m.release()
    assert (m.c.debt, m.c.inflight, m.absR) == (0, 0, absr_after_release)
    assert m.take(4) == absr_after_release                                # the un-taken bytes an overflow left are handed out again
    ring.close()


def test_reference_mode_restarts_at_zero_and_clamps_without_moving_rpos(ring_check):
    ring = ring_check()
    ring.cmd("new 16 %d" % REFERENCE)
    a, b, c3 = lcg_bytes(10, 1), lcg_bytes(8, 2), lcg_bytes(6, 3)
    ring.cmd("push 10 1")
    c, rest = ring.cmd("pop 4")
    assert rest[0] == "4" and bytes.fromhex(rest[1]) == a[:4] and (c.rpos, c.wpos, c.size) == (4, 10, 6)
    c, _ = ring.cmd("push 8 2")                                           # does not fit before the end: restarts at offset 0, no split copy
    assert (c.rpos, c.wpos, c.size, c.dropped) == (4, 8, 14, 0)
    assert ring.peek(0, 16) == b + a[8:10] + bytes(6)
    c, _ = ring.cmd("push 6 3")                                           # 14 + 6 > 16: the count is clamped, rpos stays
    assert (c.rpos, c.wpos, c.size, c.dropped) == (4, 14, 16, 4)
    assert ring.peek(0, 16) == b + c3 + bytes(2)
    c, rest = ring.cmd("pop 16")                                          # the reader sees new data where it expected old
    assert rest[0] == "16" and bytes.fromhex(rest[1]) == b[4:] + c3 + bytes(2) + b[:4] and (c.rpos, c.size) == (4, 0)
    ring.close()
