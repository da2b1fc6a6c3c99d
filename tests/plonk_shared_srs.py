"""TEST TOOLING -- trapdoor PLONK keys that share an SRS, proofs forged for them, and a model of the class layout of the aggregate check on
PLONK key sets (include/zkv_plonk_set_agg.h, csrc/zkv_gset_layout.h pset_agg_choose).

Every key plonk_trapdoor_keys.make_key makes draws its own tau.  A key's discrete logs do not depend on tau, so a key of a shared SRS is
a make_key key whose tau and [tau]_2 are replaced by the class's before forging (forge reads vk['tau']).  Parity unpinned by
construction (the reference holds no PLONK code): every verdict used as an expectation is plonk_model.plonk_verify's."""
import functools

import numpy as np

import plonk_trapdoor_keys as T
import spec_model as m

R = T.R


@functools.lru_cache(maxsize=None)
def class_tau(cls):
    return T.rng_for('plonk-shared-srs-tau', cls).randrange(2, R)


@functools.lru_cache(maxsize=None)
def _g2_tau(cls):
    return m.g2_mul(m.G2_GEN, class_tau(cls))


@functools.lru_cache(maxsize=None)
def key(cls, nb, nc, tag=0):
    """The trapdoor key (nb public inputs, nc commitments; `tag` tells keys of one shape apart) of SRS class `cls`."""
    vk = dict(T.make_key(T.rng_for('plonk-shared-srs-key', nb, nc, tag), nb, nc))
    vk['tau'], vk['g2_tau'] = class_tau(cls), _g2_tau(cls)
    return vk


def key_bytes(cls, nb, nc, tag=0):
    return T.vk_bytes(key(cls, nb, nc, tag))


@functools.lru_cache(maxsize=None)
def valid(cls, nb, nc, tag, j):
    """(proof bytes, public inputs as ints) of the j-th valid proof forged for key (cls, nb, nc, tag)."""
    pub = T.inputs(('shared-srs', cls, nb, nc, tag, j), nb)
    return T.forge(key(cls, nb, nc, tag), pub, T.rng_for('plonk-shared-srs-proof', cls, nb, nc, tag, j)), tuple(pub)


def rows_of(cls, nb, nc, tag, n_valid, ps, ins):
    """n_valid forged proofs of one key as padded numpy rows: proofs (n_valid, ps), public inputs (n_valid, ins // 32, 32)."""
    P = np.zeros((n_valid, ps), np.uint8)
    Q = np.zeros((n_valid, max(ins // 32, 1), 32), np.uint8)
    for j in range(n_valid):
        proof, pub = valid(cls, nb, nc, tag, j)
        P[j, :len(proof)] = np.frombuffer(proof, np.uint8)
        for b, x in enumerate(pub):
            Q[j, b] = np.frombuffer(x.to_bytes(32, 'big'), np.uint8)
    return P, Q[:, :ins // 32]


def damage_at_the_pairing(P, rows):
    """eval_l+1 of plonk_trapdoor_keys.apply_case on rows `rows` of the proof array P: the claimed l(zeta) (word 12) plus one mod R passes
    every range and curve check and fails the pairing equation only."""
    for i in rows:
        v = (int.from_bytes(P[i, 384:416].tobytes(), 'big') + 1) % R
        P[i, 384:416] = np.frombuffer(v.to_bytes(32, 'big'), np.uint8)


# ---------------------------------------------------------------- the class layout (a model of pset_agg_choose, written from the contract)
def unit(sub):
    return max(64, sub)


def layout(cnt, cls, capable, sub):
    """cnt[k]: proofs of key k; cls[k]: its class; capable[c].  Key groups on 64-slot boundaries, ordered class by class (capable classes
    first, each kind in class order), every class region from a multiple of A = max(64, sub) to the next.  -> dict(start (per key), cbeg,
    cend (per class), R (end of the capable regions), slots)."""
    A = unit(sub)
    n_cls = len(capable)
    start = [0] * len(cnt)
    cbeg, cend = [0] * n_cls, [0] * n_cls
    s = Rr = 0
    for want in (True, False):
        for c in range(n_cls):
            if bool(capable[c]) != want:
                continue
            cbeg[c] = s
            for k in range(len(cnt)):
                if cls[k] == c:
                    start[k] = s
                    s += (int(cnt[k]) + 63) // 64 * 64
            s = (s + A - 1) // A * A
            cend[c] = s
        if want:
            Rr = s
    return dict(start=start, cbeg=cbeg, cend=cend, R=Rr, slots=s)


def slots_of(kk, n_keys, lay):
    """The slot of every proof of a batch with key indices kk (stable within a key; -1 for an index past the set)."""
    kk = np.asarray(kk, np.int64)
    out = np.full(len(kk), -1, np.int64)
    for k in range(n_keys):
        idx = np.nonzero(kk == k)[0]
        out[idx] = lay['start'][k] + np.arange(len(idx))
    return out


def predict(kk, n_keys, cls, capable, sub):
    """(sub-batches the aggregate region holds, per proof its sub-batch id or -1 when it takes the per-proof path)."""
    kk = np.asarray(kk, np.int64)
    cnt = [int((kk == k).sum()) for k in range(n_keys)]
    lay = layout(cnt, cls, capable, sub)
    sl = slots_of(kk, n_keys, lay)
    sb = np.where((sl >= 0) & (sl < lay['R']), sl // sub, -1)
    return lay['R'] // sub, sb
