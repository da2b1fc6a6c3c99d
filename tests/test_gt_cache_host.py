"""The walk-prefix cache of the SP1 final exponentiation (csrc/zkv_gt.h), host side.

  * the selection logic the fill and tag kernels run (sample positions, the at-least-twice rule, lowest index, full cache and the cursor's
    wrap, keys that differ in one word): tests/host_cpp/test_gt_cache_select.cpp, a stand-alone program built plain and with
    AddressSanitizer and UndefinedBehaviorSanitizer;
  * the paired final_exp_prog_p with a hit, with a miss, and with a hit in one pair beside a miss in another, on the Miller values of the
    corpus' SP1 proofs: tests/host_sim/host_sim_gt_cache.cpp.  Each run must give the verdict and the u (hence u / conj(u)) of the walk
    without a cache.  The emulation plays one lane pair at a time (the wave-wide window skip is per lane there), and its tables are
    synthetic -- rows of the real geometry, entries set by the test: the property holds for any entries.  Accepting runs are constructed
    (Miller value 1 and two windows whose entries are a and -a: u = (a + w)(-a + w) lies in Fp6, so u == conj(u))."""
import ctypes as C
import os
import random
import subprocess

import pytest

import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'stylus_zkvm_verifiers_amd', 'csrc')
SELECT_SRC = os.path.join(HERE, 'host_cpp', 'test_gt_cache_select.cpp')
H = bytes.fromhex
W = 20
NW0, NW1 = 3, 2                                          # windows of the emulation's two signals: 5 sparse rows
RINV = pow(1 << 261, -1, m.P)


@pytest.mark.parametrize('flags,name', [([], 'plain'), (['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'san')])
def test_selection_logic(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g'] + flags + ['-o', exe, SELECT_SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, (out.stdout.decode()[-2000:], out.stderr.decode()[-2000:])
    assert not out.stderr, out.stderr.decode()[-2000:]
    last = out.stdout.decode().splitlines()[-1].split()
    assert last[0] == 'ok' and int(last[1]) > 400


def _build(name, extra):
    src = os.path.join(HERE, 'host_sim', name + '.cpp')
    lib = os.path.join(HERE, 'host_sim', 'lib%s.so' % name)
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-Wno-unknown-pragmas'] + extra + ['-o', lib, src])
    return C.CDLL(lib)


@pytest.fixture(scope='module')
def sim():
    hs = _build('host_sim', [])
    hs.hs_prepare.restype = C.c_void_p
    gc = _build('host_sim_gt_cache', ['-pthread'])
    gc.hs_gtc_run.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert gc.hs_gtc_init(NW0, NW1) == 0
    return hs, gc


def digits(s, n):
    out = []
    for j in range(n):
        w = (s >> (W * j)) & ((1 << W) - 1)
        c = (s >> (W * j - 1)) & 1 if j else 0
        out.append(w + c - ((w >> 19) << W))
    assert sum(d << (W * j) for j, d in enumerate(out)) == s
    return out


def words(x, n=8):
    return [(x >> (32 * k)) & 0xFFFFFFFF for k in range(n)]


class Tables:
    """Entries of the emulation's tables, set on first use: six seeded residues per entry (a0 a1 a2, (c0, c1) each)."""
    def __init__(self, gc):
        self.gc, self.rng, self.have = gc, random.Random(0x6CAC4E), {}

    def put(self, row, mag, vals=None):
        if (row, mag) in self.have and vals is None:
            return self.have[(row, mag)]
        vals = vals or [self.rng.randrange(1, m.P) for _ in range(6)]
        buf = (C.c_uint32 * 48)(*[w for v in vals for w in words(v)])
        assert self.gc.hs_gtc_set_entry(row, mag, buf) == 0
        self.have[(row, mag)] = vals
        return vals

    def cover(self, s0, s1):
        for sig, s, nw in ((0, s0, NW0), (1, s1, NW1)):
            for j, d in enumerate(digits(s, nw)):
                if d:
                    self.put((NW0 if sig else 0) + j, abs(d))


def sc16(s0, s1):
    return (C.c_uint32 * 16)(*(words(s0) + words(s1)))


def canon(u96):
    return [sum(int(u96[8 * i + k]) << (32 * k) for k in range(8)) * RINV % m.P for i in range(12)]


def run(gc, inp, s0, s1, use_cache):
    """(verdict, tag, canonical u) of one pair."""
    t, fl, norm, b = inp
    u = (C.c_uint32 * 96)()
    r = gc.hs_gtc_run(t, fl, norm, b, sc16(s0, s1), 1 if use_cache else 0, u)
    assert r >= 0, r
    return r & 0xFF, r >> 8, canon(u)


def fill(gc, s0):
    slot = gc.hs_gtc_fill((C.c_uint32 * 8)(*words(s0)))
    assert 0 <= slot < 4
    return slot


def state(gc):
    out = (C.c_uint32 * 3)()
    gc.hs_gtc_state(out)
    return dict(valid=out[0], fills=out[1], cursor=out[2])


@pytest.fixture(scope='module')
def inputs(sim, verify_corpus):
    """Miller inputs of the corpus' SP1 proofs that reach the pairing (every one of them is rejected here: the tables are synthetic), with
    their signals cut to the emulation's windows, plus constructed accepting inputs with the Miller value 1."""
    hs, gc = sim
    tab = Tables(gc)
    rows = []
    for c in verify_corpus['cases']:
        if c['vm'] != 'sp1' or c['status'] not in (0, 1):
            continue
        pvh = m.sp1_hash_public_values(H(c['public_values']))
        fl = C.c_uint32(0); norm = (C.c_uint32 * 48)(); b = (C.c_uint32 * 32)()
        t = hs.hs_prepare(1, None, None, H(c['proof'])[4:], H(c['vkey']), m.be32(pvh), C.byref(fl), norm, b)
        if not t:
            continue
        s0 = int.from_bytes(H(c['vkey']), 'big') % (1 << (W * NW0 - 1))
        s1 = pvh % (1 << (W * NW1 - 1))
        tab.cover(s0, s1)
        rows.append(((t, fl.value, norm, b), s0, s1, 0))
        if len(rows) == 6:
            break
    assert len(rows) >= 3
    # accepts: Miller value 1, one digit d0 in window j of signal 0, one digit e in window 0 of signal 1 whose entry is minus the other
    for j, d0, e in ((0, 77, 1001), (2, (1 << 18) + 5, 1002)):
        a = tab.put(j, d0)
        tab.put(NW0, e, [(m.P - v) % m.P for v in a])
        rows.append(((None, 0, None, None), d0 << (W * j), e, 1))
    # the same signal 0 with another signal 1: rejected
    tab.cover(77, 1003)
    rows.append(((None, 0, None, None), 77, 1003, 0))
    return tab, rows


def test_hit_and_miss_give_the_uncached_walk(sim, inputs):
    _, gc = sim
    tab, rows = inputs
    base = []
    for inp, s0, s1, want in rows:
        v, tag, u = run(gc, inp, s0, s1, False)
        assert tag == 0 and v == want, (hex(s0), hex(s1))
        base.append((v, u))
    assert any(v for v, _ in base) and not all(v for v, _ in base)
    for k, (inp, s0, s1, _) in enumerate(rows):
        # miss: the cache holds another key (one bit away in the last word the emulation's windows reach)
        gc.hs_gtc_reset()
        other = s0 ^ (1 << 40)
        tab.cover(other, 0)
        fill(gc, other)
        v, tag, u = run(gc, inp, s0, s1, True)
        assert tag == 0 and (v, u) == base[k], ('miss', k)
        # miss against an empty cache
        gc.hs_gtc_reset()
        v, tag, u = run(gc, inp, s0, s1, True)
        assert tag == 0 and (v, u) == base[k], ('empty', k)
        # hit, in every slot in turn
        for slot in range(4):
            gc.hs_gtc_reset()
            for pad in range(slot):                              # move the cursor: `slot` other keys first
                o = s0 ^ ((pad + 1) << 42)
                tab.cover(o, 0)
                assert fill(gc, o) == pad
            assert fill(gc, s0) == slot
            v, tag, u = run(gc, inp, s0, s1, True)
            assert tag == slot + 1 and (v, u) == base[k], ('hit', k, slot)
            assert state(gc) == dict(valid=slot + 1, fills=slot + 1, cursor=(slot + 1) % 4)


def test_a_hit_pair_beside_a_miss_pair(sim, inputs):
    """One cache state, two pairs: the pair whose key is cached starts from the stored u, the other walks -- both as without a cache."""
    _, gc = sim
    tab, rows = inputs
    gc.hs_gtc_reset()
    inp_a, a0, a1, _ = rows[0]
    inp_b, b0, b1, _ = next(r for r in rows[::-1] if r[1] != a0)      # (a constructed row: its signal 0 is not the corpus vkey)
    want_a, want_b = run(gc, inp_a, a0, a1, False), run(gc, inp_b, b0, b1, False)
    slot = fill(gc, a0)
    got_a, got_b = run(gc, inp_a, a0, a1, True), run(gc, inp_b, b0, b1, True)
    assert got_a == (want_a[0], slot + 1, want_a[2]) and got_b == (want_b[0], 0, want_b[2])
    # eviction: four more keys push a0 out, its pair walks again with the same result
    for pad in range(4):
        o = b0 ^ ((pad + 1) << 42)
        tab.cover(o, 0)
        fill(gc, o)
    assert state(gc)['fills'] == 5
    got_a = run(gc, inp_a, a0, a1, True)
    assert got_a == (want_a[0], 0, want_a[2])


def test_the_stored_prefix_is_the_walk_over_signal_zero(sim, inputs):
    """u of (s0, 0) without a cache is what a hit on s0 starts from: with signal 1 = 0 the hit lane multiplies nothing at all."""
    _, gc = sim
    tab, rows = inputs
    for inp, s0, _, _ in rows[:3]:
        gc.hs_gtc_reset()
        want = run(gc, inp, s0, 0, False)
        fill(gc, s0)
        got = run(gc, inp, s0, 0, True)
        assert got[1] == 1 and (got[0], got[2]) == (want[0], want[2])
    # signal 0 = 0: the prefix is u = 1 and a hit on it changes nothing either
    gc.hs_gtc_reset()
    inp, _, s1, _ = rows[0]
    want = run(gc, inp, 0, s1, False)
    fill(gc, 0)
    got = run(gc, inp, 0, s1, True)
    assert got[1] == 1 and (got[0], got[2]) == (want[0], want[2])
