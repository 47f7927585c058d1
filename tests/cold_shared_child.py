"""Case 8 of tests/test_gpu_cold_paths.py, the child's side: a fresh process whose FIRST launch of one instantiation of the
LDS-shared greedy form (csrc/iiv_greedy.hip launch_shared: resident_of[dev] and the LDS attribute are set there, once per
process) comes from an iiv_encode on a sleeping non-blocking stream.  The encoder's first encode waits for its stream whatever
it runs (its descriptor and counter buffers grow from nothing), so the child first makes a priming call under the forced PLAIN
form -- another instantiation, the same buffers -- on the null stream, and only then forces the shared form.
`python cold_shared_child.py MODE FOURTH` prints one line,
"cold-shared <sha256 of the opcodes> <launches per form>"; the parent holds the digest to the oracle's.  inputs() is what both
sides encode."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

N_STREAMS, SEED0 = 2, 81
SLEEP_CYCLES = 200_000_000    # (the probes' sleep: the first shared launch also sets an attribute and asks for the occupancy)


def inputs(mode):
    """(main frames, aux frames, segments) of the child's one call"""
    from stream_cases import frames
    fm, fa = frames(mode, N_STREAMS, 2, 1300 + mode)
    b = 1 if mode == 1 else 0
    return fm, fa, [(0, 0, 1, 40), (1, b, 1, 30), (1, b, 0, 20)]


PRIME = [(1, 0, 1, 10), (0, 0, 1, 11), (0, 0, 0, 12)]      # the priming call: as many rounds as the cold call (cold_cases.CHILD_SEGMENTS)


def digest(ops):
    return hashlib.sha256(np.ascontiguousarray(ops, np.uint8).tobytes()).hexdigest()


def main(argv):
    mode, fourth = int(argv[1]), bool(int(argv[2]))
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "ii-vision_amd", "transcoder"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ctypes as C
    import torch
    import _iiv_native as native
    import encode_harness as H
    import oracle
    oracle.build()
    fm, fa, segments = inputs(mode)
    _, dm = native.cie2000_matrix(oracle.PALETTE_RGB[5])
    tables = (native.build_table(mode, dm, True), native.build_store_table(mode, dm), dm)
    seeds = [H.seed_states(oracle, SEED0 + i, SEED0 + 100 + i) for i in range(N_STREAMS)]    # (the oracle's seeding: host only)
    enc = H.make_encoder(native, tables, mode, n_streams=N_STREAMS, kernel="plain", rng=seeds,
                         **({"fourth": True} if fourth else {}))
    d_main, d_aux = torch.from_numpy(fm).cuda(), torch.from_numpy(fa).cuda()
    enc.profile(True)
    enc.encode(d_main, d_aux if mode == 1 else None, PRIME)
    enc.check()
    torch.cuda.synchronize()
    primed = enc.launch_forms()
    assert primed["plain"] == len(PRIME) == sum(primed.values()), primed      # no shared-form launch yet in this process
    enc.set_greedy_kernel("shared")
    enc.profile(True)
    total = sum(s[3] for s in segments)
    ops = torch.zeros((N_STREAMS, total, 6), dtype=torch.uint8, device="cuda")
    segs = native.segment_array(segments)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()                    # torch's streams are non-blocking: the null stream does not order this one
    with torch.cuda.stream(side):
        torch.cuda._sleep(SLEEP_CYCLES)
        native.check(native.lib().iiv_encode(enc._h, C.c_void_p(d_main.data_ptr()), C.c_void_p(d_aux.data_ptr() if mode == 1 else 0), 2,
                                             segs, len(segments), C.c_void_p(ops.data_ptr()), C.c_void_p(side.cuda_stream)))
        busy = not side.query()
    side.synchronize()
    enc.check()
    print("cold-shared %s %s %d" % (digest(ops.cpu().numpy()), json.dumps(enc.launch_forms(), sort_keys=True), int(busy)), flush=True)
    enc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
