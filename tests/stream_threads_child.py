"""The child of tests/test_gpu_streams.py::test_gpu_two_host_threads_first_call_included: two host threads meet at a
barrier before the library's very first device call, then each runs 20 rounds on a stream of its own -- one
rhp_parse_batch under IMPL_DFA followed by rhp_write_responses, the other rhp_parse_batch under IMPL_DFA_LATE followed
by rhp_classify_batch (ctypes releases the GIL, so the calls overlap).  Every round is checked against the host twins.
Prints OK."""
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np   # noqa: E402
import torch   # noqa: E402

import libreactorng_amd as rhp   # noqa: E402
import stream_sets as ss   # noqa: E402
from test_gpu_streams import Buffers   # noqa: E402

ROUNDS = 20


def worker(impl, parse, second, barrier, errors):
    try:
        stream = torch.cuda.Stream()
        cases = ((parse, "A"), (second, "B"))
        bufs = [Buffers(c, w, w) for c, w in cases]
        torch.cuda.synchronize()
        barrier.wait(timeout=60)
        rhp.lib().rhp_set_impl(impl)
        for r in range(ROUNDS):
            for (c, w), b in zip(cases, bufs):
                with torch.cuda.stream(stream):
                    b.refill(w)
                c.launch(b.T, c.side(w), stream)
            stream.synchronize()
            for (c, w), b in zip(cases, bufs):
                b.check(w, f"thread impl {impl} round {r}: {c.name}")
    except BaseException as e:   # (reported by the main thread)
        errors.append(f"impl {impl}: {type(e).__name__}: {e}")
        barrier.abort()


def main():
    assert torch.cuda.is_available()
    rhp.lib()
    for c in (ss.BY_NAME["write_responses"], ss.BY_NAME["classify_batch"]):   # the twins, before the threads start
        c.side("B")
    parses = [ss.ParseBatch(rhp.MODE_PHR), ss.ParseBatch(rhp.MODE_PHR)]
    for p in parses:
        p.side("A")
    barrier, errors = threading.Barrier(2), []
    threads = [threading.Thread(target=worker, args=(rhp.IMPL_DFA, parses[0], ss.BY_NAME["write_responses"], barrier, errors)),
               threading.Thread(target=worker, args=(rhp.IMPL_DFA_LATE, parses[1], ss.BY_NAME["classify_batch"], barrier, errors))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        print("\n".join(errors))
        return 1
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
