"""The 16-lane cooperative Poseidon permutation (csrc/poseidon.cuh poseidon_permute_coop16) on the GPU: the function itself through
sbn_poseidon_permute_coop_batch against the host's plain-definition permutation, at counts that leave waves and workgroups partly
filled, and the Merkle kernels that run it (merkle_subtree_kernel, merkle_level_coop_kernel, the levels on either side of the
lane-per-parent crossover) through commit_values against the oracle's cap."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module")
def gpu(S):
    if S.lib().sbn_device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the MI355X box (there is no CPU fallback)")
    return S


@pytest.fixture(scope="module")
def states(golden):
    """KAT inputs, the constant states, the fold's carry / borrow edges, one non-zero word per position, 1,000 random states."""
    kat = [[int(x, 16) for x in v["input"]] for v in golden["poseidon_kat"]["vectors"]]
    rows = list(kat)
    for w in (0, P - 1, (1 << 32) - 1, 1 << 32, P - (1 << 32)):
        rows.append([w] * 12)
    for pos in range(12):                               # a wrong rotation of a lane's constant row moves this word's weight
        rows.append([0x0123456789ABCDEF + pos if k == pos else 0 for k in range(12)])
    for pos in range(12):                               # the edges in one position, the other words at the opposite edge
        rows.append([(1 << 32) - 1 if k == pos else P - (1 << 32) for k in range(12)])
    rng = np.random.default_rng(2024)
    st = np.concatenate([np.array(rows, dtype=np.uint64), rng.integers(0, P, size=(1000, 12), dtype=np.uint64)])
    assert (st < P).all()
    return {"kat": len(kat), "in": st}


@pytest.fixture(scope="module")
def expected(S, states):
    """The host's plain definition of the permutation, computed once."""
    return S.poseidon_permute_host(states["in"], use_definition=True)


def test_coop_permutation_matches_the_host_definition(gpu, golden, states, expected):
    out = gpu.poseidon_permute_coop_batch(states["in"])
    bad = np.flatnonzero((out != expected).any(axis=1))
    assert bad.size == 0, f"first differing state: {bad[0]}"
    kat = golden["poseidon_kat"]["vectors"]
    assert [[int(x) for x in r] for r in out[:states["kat"]]] == [[int(x, 16) for x in v["output"]] for v in kat]
    assert (out < P).all()                              # every lane returns the canonical value
    with pytest.raises(gpu.SbnError) as e:              # non-canonical input is refused
        gpu.poseidon_permute_coop_batch(np.full((1, 12), P, dtype=np.uint64))
    assert e.value.code == -2


@pytest.mark.parametrize("count", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65])
def test_coop_permutation_partial_groups(gpu, states, expected, count):
    """4 groups per wave, 16 per workgroup: the last wave and the last workgroup run with idle groups, whose lanes still execute the
    permutation (loads and stores are predicated, the call is not).  The states are taken from the end of the shared set, so the last
    group of every count holds a random state."""
    n = len(states["in"])
    out = gpu.poseidon_permute_coop_batch(states["in"][n - count:])
    assert out.shape == (count, 12)
    assert np.array_equal(out, expected[n - count:])


@pytest.mark.parametrize("n", [512, 1024, 8192, 16384, 32768])
def test_tree_kernels_match_the_oracle_cap(gpu, O, n):
    """Five columns, so that leaves are hashed; rate_bits 1: 2^10, 2^11, 2^14, 2^15 and 2^16 leaves.  1,024 leaves finish in one
    workgroup after one five-level launch; 2^14 leaves and more take both five-level subtree launches; the 2^15-leaf tree starts
    with the 16,384-parent level, the widest that runs 16 lanes per parent (merkle_level_coop_kernel), and the 2^16-leaf tree with
    the 32,768-parent level, the narrowest that runs one lane per parent: the levels on either side of the crossover in
    tree_build_inner.  cap_height 4 and 1 end the last launch at different depths."""
    rng = np.random.default_rng(7000 + n)
    cols = rng.integers(0, P, size=(5, n), dtype=np.uint64)
    for cap_height in (4, 1):
        cap, _, _ = gpu.commit_values(cols, cap_height=cap_height)
        rcap, _, _ = O.commit_values(cols, cap_height=cap_height)
        assert cap.shape == (1 << cap_height, 4)
        assert np.array_equal(cap, rcap), cap_height
