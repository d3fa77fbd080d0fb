#!/usr/bin/env python3
"""Writes tests/golden/decode_chunked.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every stream of every set of tests/decode_chunked_sets.py the compiled
reference's phr_decode_chunked is called directly, through ctypes, piece after
piece on a private copy of each piece, the decoder going from one call to the
next as the reference left it.  A record is one call: the piece before, the
decoder before, the piece after, ret, *bufsz and the decoder after.  Equal calls
(the same bytes and decoder before: the first halves of two cuts, a prefix) are
one record; a set lists its calls as record indices.

The file is flat, so that the stand-alone C test
(tests/decode_chunked_host_test.c) reads it as well: np.savez, not compressed; S
sets, I calls, R records.
  set_name   str [S]       set_start u64 [S]  the byte the set's batch packs its pieces from
  set_lo     u32 [S + 1]   set s holds calls [set_lo[s], set_lo[s + 1])
  item_rec   u32 [I]       the call's record
  item_first u8 [I]        1: the first call of its stream (else the decoder before is the previous call's after)
  rec_lo     u64 [R + 1]   record r's piece is before / after [rec_lo[r], rec_lo[r + 1])
  before, after  u8        dec_before, dec_after  u8 [R * 16] (rhp_chunked_t)
  ret        i64 [R]       size  u64 [R]
usage: python tests/golden/make_golden_decode_chunked.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import decode_chunked_sets as ds  # noqa: E402

GOLDEN = os.path.join(HERE, "decode_chunked.npz")


def reference():
    ref = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref.so"))
    ref.phr_decode_chunked.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    ref.phr_decode_chunked.restype = ctypes.c_ssize_t
    return ref


def reference_call(ref, decoder: bytes, piece: bytes):
    """(ret, *bufsz, decoder after, piece after) of one phr_decode_chunked call; the piece in an allocation of
    exactly its size"""
    d = np.frombuffer(decoder, dtype=np.uint8).copy()
    p = np.frombuffer(piece, dtype=np.uint8).copy()
    sz = ctypes.c_size_t(len(piece))
    ret = ref.phr_decode_chunked(d.ctypes.data, p.ctypes.data, ctypes.byref(sz))
    return int(ret), int(sz.value), d.tobytes(), p.tobytes()


def main():
    ref = reference()
    recs, index = [], {}
    names, starts, set_lo, item_rec, item_first = [], [], [0], [], []
    for name, start, streams in ds.all_sets():
        rets = []
        for s in streams:
            dec = ds.fresh_decoder(s)
            for r, piece in enumerate(s.pieces):
                key = (dec, piece)
                if key not in index:
                    index[key] = len(recs)
                    recs.append((piece, dec) + reference_call(ref, dec, piece))
                item_rec.append(index[key])
                item_first.append(int(r == 0))
                _, _, ret, _, dec, _ = recs[index[key]]
                rets.append(ret)
        names.append(name)
        starts.append(start)
        set_lo.append(len(item_rec))
        rets = np.array(rets)
        print(f"{name}: {len(streams)} streams, {len(rets)} calls: {int((rets >= 0).sum())} complete, "
              f"{int((rets == -1).sum())} x -1, {int((rets == -2).sum())} x -2")
    rec_lo = np.cumsum([0] + [len(r[0]) for r in recs]).astype(np.uint64)
    cat = lambda k: np.frombuffer(b"".join(r[k] for r in recs), dtype=np.uint8)
    out = dict(set_name=np.array(names), set_start=np.array(starts, dtype=np.uint64), set_lo=np.array(set_lo, dtype=np.uint32),
               item_rec=np.array(item_rec, dtype=np.uint32), item_first=np.array(item_first, dtype=np.uint8), rec_lo=rec_lo,
               before=cat(0), after=cat(5), dec_before=cat(1), dec_after=cat(4),
               ret=np.array([r[2] for r in recs], dtype=np.int64), size=np.array([r[3] for r in recs], dtype=np.uint64))
    np.savez(GOLDEN, **out)
    print(f"{GOLDEN}: {len(names)} sets, {len(item_rec)} calls, {len(recs)} records, {int(rec_lo[-1])} piece bytes, "
          f"{os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
