"""RISC Zero set-inclusion receipts (include/zkv_risc0_set_inclusion.h): one Groth16 root seal proves a Merkle root, every claim under it
carries a keccak-256 Merkle path.  The paths are hashed on the device, claims that share a root seal share one pairing check, and roots
submitted once are remembered.  PARITY UNPINNED: the reference holds no set verifier; the rules are the header's."""
import ctypes as C

import numpy as np

from . import _lib
from .errors import STATUS_OK

STORED = 0xFFFFFFFF             # ZKV_SETINCL_STORED: the claim names no root seal, its root is looked up among the submitted roots
MAX_DEPTH = 64                  # ZKV_SETINCL_MAX_DEPTH
MAX_ROOTS = 4096                # ZKV_SETINCL_MAX_ROOTS
KEY_BYTES = 448 + 64 * 6        # a key with n_ic = 6 in zkv_groth16_ctx_create's layout

_P, _SZ, _B = C.c_void_p, C.c_size_t, C.c_char_p
# declared in include/zkv_risc0_set_inclusion.h (_lib.SYMBOLS mirrors zkv.h alone)
SYMBOLS = {
    'zkv_risc0_setincl_create': (C.c_void_p, [_B, _B, _B, C.c_int]),
    'zkv_risc0_setincl_create_keyed': (C.c_void_p, [_B, _B, _B, _B, _B, C.c_int]),
    'zkv_risc0_setincl_verify_batch': (C.c_int, [_P, _SZ, _B, _B, _B, _P, _P, _SZ, _B, _P, _P, _P]),
    'zkv_risc0_setincl_verify_integrity_batch': (C.c_int, [_P, _SZ, _B, _B, _P, _P, _SZ, _B, _P, _P, _P]),
    'zkv_risc0_setincl_verify_batch_dev': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _SZ, _P, _SZ, _P, _P, _P, _P]),
    'zkv_risc0_setincl_submit_root': (C.c_int, [_P, _B, _B, _SZ, C.POINTER(C.c_uint8), _B]),
    'zkv_risc0_setincl_has_root': (C.c_int, [_P, _B]),
    'zkv_risc0_setincl_get_selector': (C.c_int, [_P, _B]),
    'zkv_risc0_setincl_last_counts': (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    'zkv_risc0_setincl_seal_encode': (_SZ, [_P, _B, _SZ, _B, _SZ, _B, _SZ]),
    'zkv_risc0_setincl_seal_decode': (C.c_int, [_P, _B, _SZ, C.POINTER(C.c_uint8), _B, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_SZ)]),
    'zkv_diag_setincl_roots': (C.c_int, [_P, _SZ, _B, _B, _B, _P, _SZ, _P]),
}

_bound = None


def lib():
    """The library with this header's symbols bound (AttributeError when one is not exported)."""
    global _bound
    L = _lib.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def _cat32(items, what):
    for x in items:
        if len(x) != 32:
            raise ValueError('%s must be 32 bytes' % what)
    return b''.join(bytes(x) for x in items) + b'\0'


def _paths(paths):
    """Ragged paths (each a list of 32-byte siblings, or their concatenation) -> blob, uint32 offsets in sibling units."""
    flat = [p if isinstance(p, (bytes, bytearray)) else b''.join(bytes(s) for s in p) for p in paths]
    for p in flat:
        if len(p) % 32:
            raise ValueError('a path is a whole number of 32-byte siblings')
    off = np.zeros(len(flat) + 1, dtype=np.uint64)
    if flat:
        off[1:] = np.cumsum([len(p) // 32 for p in flat], dtype=np.uint64)
    if int(off[-1]) > 0xFFFFFFFF:
        raise ValueError('more than 2^32 - 1 siblings in one call')
    return b''.join(bytes(p) for p in flat) + b'\0', off.astype(np.uint32)


def _seals(root_seals):
    off = np.zeros(len(root_seals) + 1, dtype=np.uint64)
    if len(root_seals):
        off[1:] = np.cumsum([len(s) for s in root_seals], dtype=np.uint64)
    return b''.join(bytes(s) for s in root_seals) + b'\0', off


class RiscZeroSetInclusionVerifier:
    """A set verifier for one set-builder image id behind one inner root verifier (control_root, bn254_control_id): the built-in RISC
    Zero key, or -- vk_words (n_ic = 6, the reference's word order) and root_selector given -- a caller-supplied key in the RISC Zero
    convention."""

    def __init__(self, control_root, bn254_control_id, set_builder_image_id, vk_words=None, root_selector=None, device=0):
        for name, v in (('control_root', control_root), ('bn254_control_id', bn254_control_id), ('set_builder_image_id', set_builder_image_id)):
            if len(v) != 32:
                raise ValueError('%s must be 32 bytes' % name)
        if (vk_words is None) != (root_selector is None):
            raise ValueError('vk_words and root_selector come together')
        self._L = lib()
        if vk_words is None:
            self._h = self._L.zkv_risc0_setincl_create(bytes(control_root), bytes(bn254_control_id), bytes(set_builder_image_id), device)
        else:
            if len(vk_words) != KEY_BYTES:
                raise ValueError('the root key takes %d bytes (n_ic = 6)' % KEY_BYTES)
            if len(root_selector) != 4:
                raise ValueError('root_selector must be 4 bytes')
            self._h = self._L.zkv_risc0_setincl_create_keyed(bytes(vk_words), bytes(root_selector), bytes(control_root), bytes(bn254_control_id),
                                                             bytes(set_builder_image_id), device)
        if not self._h:
            raise MemoryError('zkv_risc0_setincl_create')

    def close(self):
        if getattr(self, '_h', None):
            self._L.zkv_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def handle(self):
        return self._h

    def get_selector(self):
        """The selector of the on-chain seal form."""
        o = C.create_string_buffer(4)
        _lib.check(self._L.zkv_risc0_setincl_get_selector(self._h, o), 'zkv_risc0_setincl_get_selector')
        return o.raw

    # ---- batches, host buffers
    def _batch(self, first, second, paths, root_idx, root_seals):
        n = len(first)
        for name, v in (('paths', paths), ('root_idx', root_idx)) + ((('journal_digests', second),) if second is not None else ()):
            if len(v) != n:
                raise ValueError('%s has %d entries for a batch of %d claims' % (name, len(v), n))
        blob, off = _paths(paths)
        ridx = np.ascontiguousarray(np.asarray(root_idx, dtype=np.uint64).astype(np.uint32))
        sblob, soff = _seals(root_seals)
        st = np.zeros(n, dtype=np.uint8); rv = np.zeros((n, 4), dtype=np.uint8)
        if second is not None:
            rc = self._L.zkv_risc0_setincl_verify_batch(self._h, n, _cat32(first, 'image_id'), _cat32(second, 'journal_digest'), blob, off.ctypes.data,
                                                        ridx.ctypes.data, len(root_seals), sblob, soff.ctypes.data, st.ctypes.data, rv.ctypes.data)
        else:
            rc = self._L.zkv_risc0_setincl_verify_integrity_batch(self._h, n, _cat32(first, 'claim_digest'), blob, off.ctypes.data, ridx.ctypes.data,
                                                                  len(root_seals), sblob, soff.ctypes.data, st.ctypes.data, rv.ctypes.data)
        _lib.check(rc, 'zkv_risc0_setincl_verify_batch')
        return st, rv

    def verify_batch(self, image_ids, journal_digests, paths, root_idx, root_seals):
        """`verify` of n claims: claim i has path paths[i] and names root seal root_seals[root_idx[i]] (STORED: its root is looked up among
        the submitted roots).  One status byte per claim (errors.STATUS_*) and the received selector of mismatching root seals."""
        return self._batch(image_ids, journal_digests, paths, root_idx, root_seals)

    def verify_integrity_batch(self, claim_digests, paths, root_idx, root_seals):
        return self._batch(claim_digests, None, paths, root_idx, root_seals)

    def verify_batch_dev(self, n, d_image_ids, d_journal_digests, d_path_blob, d_path_off, n_siblings, d_root_idx, m, d_root_seals, d_status,
                         d_recv=0, stream=0):
        """Everything resident in HBM (device pointers as ints): root seals as m rows of 260 bytes; d_journal_digests = 0 selects
        verify_integrity (d_image_ids then holds claim digests).  The call synchronises `stream` once per chunk of 2^20 claims (it reads
        the number of root jobs back); the rest is asynchronous."""
        _lib.check(self._L.zkv_risc0_setincl_verify_batch_dev(self._h, n, d_image_ids, d_journal_digests or None, d_path_blob or None, d_path_off, n_siblings,
                                                              d_root_idx, m, d_root_seals or None, d_status, d_recv or None, stream or None),
                   'zkv_risc0_setincl_verify_batch_dev')

    # ---- submitted roots
    def submit_root(self, root, seal):
        """(status, received selector) of the inner verifier for (seal, ID, sha256(ID || root)); the root is remembered when that is OK."""
        if len(root) != 32:
            raise ValueError('root must be 32 bytes')
        st = C.c_uint8(0); rv = C.create_string_buffer(4)
        _lib.check(self._L.zkv_risc0_setincl_submit_root(self._h, bytes(root), bytes(seal), len(seal), C.byref(st), rv), 'zkv_risc0_setincl_submit_root')
        return int(st.value), rv.raw

    def has_root(self, root):
        if len(root) != 32:
            raise ValueError('root must be 32 bytes')
        r = self._L.zkv_risc0_setincl_has_root(self._h, bytes(root))
        if r < 0:
            _lib.check(r, 'zkv_risc0_setincl_has_root')
        return bool(r)

    def last_counts(self):
        """(claims, root-seal verifications actually run, stored-root lookups) of the most recent batch call."""
        out = (C.c_uint64 * 3)()
        _lib.check(self._L.zkv_risc0_setincl_last_counts(self._h, out), 'zkv_risc0_setincl_last_counts')
        return int(out[0]), int(out[1]), int(out[2])

    def synchronize(self):
        _lib.check(self._L.zkv_ctx_synchronize(self._h), 'zkv_ctx_synchronize')

    # ---- the on-chain form
    def encode_seal(self, path, root_seal):
        p = path if isinstance(path, (bytes, bytearray)) else b''.join(bytes(s) for s in path)
        if len(p) % 32:
            raise ValueError('a path is a whole number of 32-byte siblings')
        need = self._L.zkv_risc0_setincl_seal_encode(self._h, bytes(p), len(p) // 32, bytes(root_seal), len(root_seal), None, 0)
        if not need:
            raise ValueError('zkv_risc0_setincl_seal_encode refuses the arguments')
        out = C.create_string_buffer(need)
        self._L.zkv_risc0_setincl_seal_encode(self._h, bytes(p), len(p) // 32, bytes(root_seal), len(root_seal), out, need)
        return out.raw

    def decode_seal(self, seal):
        """(status, received selector, path, root seal): path and root seal are None unless the status is OK."""
        st = C.c_uint8(0); rv = C.create_string_buffer(4)
        at, k, rat, rlen = _SZ(0), _SZ(0), _SZ(0), _SZ(0)
        seal = bytes(seal)
        _lib.check(self._L.zkv_risc0_setincl_seal_decode(self._h, seal, len(seal), C.byref(st), rv, C.byref(at), C.byref(k), C.byref(rat), C.byref(rlen)),
                   'zkv_risc0_setincl_seal_decode')
        if st.value != STATUS_OK:
            return int(st.value), rv.raw, None, None
        return 0, rv.raw, seal[at.value:at.value + 32 * k.value], seal[rat.value:rat.value + rlen.value]

    def verify_seals(self, seals, image_ids, journal_digests):
        """`verify` of on-chain-form seals: decoded on the host, byte-identical root seals share one root index, empty root seals use the
        submitted roots; then one batch call.  Seals that do not decode are answered here (INVALID_PROOF_DATA / SELECTOR_MISMATCH)."""
        n = len(seals)
        if len(image_ids) != n or len(journal_digests) != n:
            raise ValueError('one image id and one journal digest per seal')
        st = np.zeros(n, dtype=np.uint8); rv = np.zeros((n, 4), dtype=np.uint8)
        keep, paths, ridx, roots, index = [], [], [], [], {}
        for i, s in enumerate(seals):
            code, recv, path, root_seal = self.decode_seal(s)
            if code != STATUS_OK:
                st[i] = code; rv[i] = np.frombuffer(recv, dtype=np.uint8)
                continue
            keep.append(i); paths.append(path)
            if not root_seal:
                ridx.append(STORED)
            else:
                if root_seal not in index:
                    index[root_seal] = len(roots); roots.append(root_seal)
                ridx.append(index[root_seal])
        if keep:
            s2, r2 = self.verify_batch([image_ids[i] for i in keep], [journal_digests[i] for i in keep], paths, ridx, roots)
            st[keep] = s2; rv[keep] = r2
        return st, rv

    def diag_roots(self, image_ids, journal_digests, paths, blob_shift=0):
        """Test only (zkv_diag_setincl_roots): root_i of every claim, n x 32 bytes; journal_digests = None: the first list holds claim digests."""
        n = len(image_ids)
        blob, off = _paths(paths)
        out = np.zeros((n, 32), dtype=np.uint8)
        _lib.check(self._L.zkv_diag_setincl_roots(self._h, n, _cat32(image_ids, 'image_id'),
                                                  _cat32(journal_digests, 'journal_digest') if journal_digests is not None else None, blob, off.ctypes.data,
                                                  blob_shift, out.ctypes.data), 'zkv_diag_setincl_roots')
        return out
