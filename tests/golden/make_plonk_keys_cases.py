"""Writes tests/golden/plonk_keys_cases.json for the PLONK-keys tests (include/zkv_plonk_keys.h).

Per (nb_public, n_c) in {0, 1, 2, 3, 8, 9, 31, 64, 128} x {0, 1}: the SHA-256 of the trapdoor key (tests/plonk_trapdoor_keys.py
derives it from its seed), the forged valid proof, and one verdict digit per case of case_names() -- oracle/plonk_model.plonk_verify's,
and the C oracle's for nb_public <= 8 (the two must agree).  Per (nb_public, n_c), nb_public in {0, 2, 9, 128}: POOL_N more valid
proofs for batch tests.  Public inputs and the tampered cases are recomputed from their names, so the file stays small.

Run from the repository root:  PYTHONPATH=oracle:tests python tests/golden/make_plonk_keys_cases.py   (about a minute)"""
import base64
import hashlib
import json
import os
import sys
from multiprocessing import Pool

import oracle_lib as ol
import plonk_trapdoor_keys as T


def verdicts(args):
    nb, nc, proof = args
    vk = T.vk_bytes(T.shape_key(nb, nc))
    model, cor = '', ''
    for name in T.case_names(nb, nc):
        v, p, q = T.apply_case(name, vk, proof, T.valid_inputs(nb, nc))
        model += '1' if T.pm.plonk_verify(T.parse_vk(v), T.pad27(p), q) else '0'
        if nb <= 8:
            cor += '1' if ol.plonk_verify(v, T.pad27(p), [x.to_bytes(32, 'big') for x in q]) else '0'
    return model, cor


def main():
    b64 = lambda b: base64.b64encode(b).decode()
    with Pool(int(os.environ.get('JOBS', '16'))) as pool:
        valid = pool.starmap(T.forge_valid, T.SHAPES)
        res = pool.map(verdicts, [(nb, nc, p) for (nb, nc), p in zip(T.SHAPES, valid)])
        pooled = pool.starmap(T.forge_pool, [(nb, nc, j) for nb, nc in T.POOL_SHAPES for j in range(T.POOL_N)])
    shapes = []
    for (nb, nc), proof, (model, cor) in zip(T.SHAPES, valid, res):
        assert model[0] == '1' and model.count('1') == 1, (nb, nc)
        assert not cor or cor == model, (nb, nc)
        shapes.append(dict(nb_public=nb, n_c=nc, vk_sha256=hashlib.sha256(T.vk_bytes(T.shape_key(nb, nc))).hexdigest(),
                           proof=b64(proof), model=model, c_oracle=cor))
        print(nb, nc, len(model), 'cases', file=sys.stderr)
    pools = [dict(nb_public=nb, n_c=nc, proofs=b64(b''.join(pooled[k * T.POOL_N:(k + 1) * T.POOL_N])))
             for k, (nb, nc) in enumerate(T.POOL_SHAPES)]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'plonk_keys_cases.json')
    with open(path, 'w') as f:
        json.dump(dict(note='make_plonk_keys_cases.py; parity unpinned (no PLONK in the reference): verdicts of oracle/plonk_model.py',
                       shapes=shapes, pool=pools), f, indent=0)
    print(path, os.path.getsize(path), 'bytes', file=sys.stderr)


if __name__ == '__main__':
    main()
