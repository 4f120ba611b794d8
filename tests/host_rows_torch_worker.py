"""Child process of tests/test_host_rows_gpu.py: rows that sit in a torch tensor on the device, handed to
Prover.load_trace_rows_device by their data_ptr().  A process of its own because torch must be imported BEFORE the library is
loaded: the torch wheel brings its own HIP runtime under the runtime's usual library name, whichever of the two is loaded first
serves both, and torch finds no device behind the other one.  Packed rows, and rows with a stride of n_cols + 5 that start 8 bytes
off torch's own alignment, the padding full of words that would be refused if they were read.  Prints "torch rows ok"."""
import os
import sys

import numpy as np
import torch

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O          # noqa: E402
import starky_bn254_amd as S    # noqa: E402

JUNK = 0x5EEDF00D5EED   # as in test_host_rows_gpu.py: what the trace buffer holds in front of every load
ios, _ = O.fq12expu64_inputs(16, 5)
trace, pi = O.fq12expu64_trace(ios)
stark = S.Fq12ExpU64Stark(16)
rows = np.ascontiguousarray(trace[:stark.num_main_columns].T)
n, nc = rows.shape
p = S.Prover(stark, stark.config(), 11)
try:
    p.load_trace(trace, pi)
    want = p.prove().words
    for pad, lead in ((0, 0), (5, 1)):
        host = np.full(lead + n * (nc + pad), 2**64 - 1, dtype=np.uint64)
        host[lead:].reshape(n, nc + pad)[:, :nc] = rows
        dev = torch.from_numpy(host.view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        assert dev.data_ptr() % 16 == 0
        p.load_trace(np.full(trace.shape, JUNK, dtype=np.uint64), pi)
        p.load_trace_rows_device(dev.data_ptr() + 8 * lead, nc + pad, nc, pi)
        assert np.array_equal(p.read_trace(), trace), (pad, lead)
        assert np.array_equal(p.prove().words, want), (pad, lead)
        del dev
finally:
    p.close()
print("torch rows ok", flush=True)
