"""What tests/test_rate_host.py (CPU: oracle proofs against the host verifier) and tests/test_rate_gpu.py (device prover against
the oracle) share: the small tables, the config rows and the oracle's proofs at a chosen rate_bits (tests/rate_oracle.py)."""
import numpy as np

import config_matrix as M

NO_PI = np.zeros(0, dtype=np.uint64)
# (cap_height, proof_of_work_bits, fri_arity_bits, fri_final_poly_bits, num_query_rounds): for_rate(3)'s row; one FRI layer more
# than the arity divides with cap height 1 and a final polynomial of one coefficient; cap height 8 with arity 2; arity 2 (a FRI leaf
# that is its own digest)
ROWS = [(4, 16, 4, 5, 28), (1, 0, 3, 2, 200), (8, 8, 1, 0, 3), (4, 16, 1, 5, 28)]
# (row, times_x): every row, and (8, 8, 1, 0, 3) also without the times-X step (fri_variant = SBN_FRI_PLAIN)
CASES = [(row, True) for row in ROWS] + [((8, 8, 1, 0, 3), False)]


def case_id(case):
    return M.case_id(case)


def make_config(S, case, rate_bits=3):
    cfg = M.make_config(S, *case)
    cfg.rate_bits = rate_bits
    return cfg


def table(S, O, name):
    """name -> (stark, oracle kind, num_io, trace): seeded, small, made on the CPU."""
    if name.startswith("g1op"):
        rows = 1 << int(name[4:] or 9)
        return S.G1Stark(), O.AIR_G1_OP, 0, O.g1op_trace(O.g1op_inputs(rows, 0)[0])
    if name == "modular":
        return S.ModularStark(), O.AIR_MODULAR, 0, O.modular_trace(O.modular_inputs(512, 7)[0])
    if name == "fq12mul":   # the widest single-operation table (9722 columns, 5328 Zs), the inputs of the rate-1 parity test
        return S.Fq12Stark(), O.AIR_FQ12_MUL, 0, O.fq12mul_trace(O.fq12mul_inputs(512, 7)[0])
    if name.startswith("lookup"):
        rows = 1 << int(name[6:] or 9)
        return S.LookupStark(), O.AIR_LOOKUP, 0, O.lookup_trace(*O.lookup_inputs(rows, 9))
    if name == "flags":
        return S.FlagStark(1), O.AIR_FLAGS, 1, O.flags_trace(O.flags_inputs(1, 11)[0])
    if name == "flagsu64":
        return S.FlagU64Stark(4), O.AIR_FLAGS_U64, 4, O.flags_u64_trace(O.flags_u64_inputs(4, 12)[0])
    raise KeyError(name)


class Proofs:
    """The oracle's proof of every (table name, case, rate_bits), made once per session."""

    def __init__(self, S, O, R):
        self.S, self.O, self.R, self.tables, self.cache = S, O, R, {}, {}

    def table(self, name):
        if name not in self.tables:
            self.tables[name] = table(self.S, self.O, name)
        return self.tables[name]

    def __call__(self, name, case, rate_bits=3):
        key = (name, case, rate_bits)
        if key not in self.cache:
            _, kind, num_io, trace = self.table(name)
            self.cache[key] = self.R.prove(kind, num_io, trace, NO_PI, rate_bits, case[0] + (case[1],))[0]
        return self.cache[key]


def product_code(S, stark, words, cfg):
    """sbn_verify's code for the proof under cfg (0 = accepted)."""
    words = np.asarray(words, dtype=np.uint64)
    try:
        S.verify_stark_proof(stark, S.Proof(words, int(words[1])), cfg)
    except S.SbnError as e:
        return e.code
    return 0
