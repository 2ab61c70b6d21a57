"""Host side of the K > 1 Hadamard chain (5120 = 5 x 1024, 3584 = 7 x 512, ...): the ABI field, the validation that
happens before any launch, the op's shape inference and `chain_supported`.  No GPU."""
import ctypes

import pytest
import torch

import quip_for_all_amd  # noqa: F401  (registers torch.ops.quip_lib.*)
from quip_for_all_amd import capi, register_lib

NULL_POINTER, BAD_SHAPE, MISALIGNED, UNSUPPORTED = -1, -2, -3, -5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    return capi.lib()


@pytest.fixture(scope="module")
def p16():
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    yield p
    del buf


def _chain_problem(p, n, z_had=None, had=None, **kw):
    """a chain problem on dummy (aligned, never dereferenced: validation returns before any launch) pointers"""
    pr = capi.HadProblem()
    pr.out, pr.pre_scale, pr.rms_weight, pr.had = p, p, p, had
    pr.in_features = pr.out_features = n
    pr.scale, pr.rms_eps, pr.z_scale = 1.0, 1e-5, 1.0
    pr.z, pr.z_post_scale, pr.z_residual, pr.h_out = p, p, p + 16, p + 32
    pr.z_had = z_had
    for k, v in kw.items():
        setattr(pr, k, v)
    return pr


def _planes_group(lib, problems, n, K):
    arr = (capi.HadProblem * len(problems))(*problems)
    return lib.quip_had_transform_planes_group(arr, len(problems), n, K, 1, None)


def test_had_problem_grew_by_one_trailing_pointer():
    names = [f[0] for f in capi.HadProblem._fields_]
    assert names[-1] == "z_had" and names[-2] == "n"
    # 10 pointers, 2 int32, 2 float | 4 pointers, 2 float, 2 int32 | the new pointer
    assert ctypes.sizeof(capi.HadProblem) == 10 * 8 + 16 + 4 * 8 + 16 + ctypes.sizeof(ctypes.c_void_p)
    assert capi.HadProblem.z_had.offset == ctypes.sizeof(capi.HadProblem) - ctypes.sizeof(ctypes.c_void_p)
    # positional constructions that stop before the new field keep working, and leave it NULL
    pr = capi.HadProblem(None, None, None, None, None, None, None, None, None, None, 8, 8, 1.0, 1e-5, None, None, None,
                         None, 1.0, 0.0, 0)
    assert pr.z_had is None and pr.n == 0


def test_chain_with_k_factor_needs_the_producers_factor(lib, p16):
    n, K = 5120, 5
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=None, had=p16)], n, K) == NULL_POINTER
    # all three consumers are checked
    good = _chain_problem(p16, n, z_had=p16, had=p16)
    assert _planes_group(lib, [good, good, _chain_problem(p16, n, z_had=None, had=p16)], n, K) == NULL_POINTER
    # the consumers' own factor is still required
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=p16, had=None)], n, K) == NULL_POINTER
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=p16, had=p16, z_post_scale=None)], n, K) == NULL_POINTER
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=p16, had=p16, h_out=None)], n, K) == NULL_POINTER


@pytest.mark.parametrize("n,K", [(5120, 20), (11008, 43), (5120, 40), (2560, 10)])
def test_tall_chains_stay_unsupported(lib, p16, n, K):
    """L <= 256 (the K-mix on the matrix cores) has no chain, with or without z_had"""
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=p16, had=p16)], n, K) == UNSUPPORTED
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=None, had=p16)], n, K) == UNSUPPORTED


def test_chain_shapes_outside_the_wide_range_are_unsupported(lib, p16):
    chain = lambda n: _chain_problem(p16, n, z_had=p16, had=p16)   # noqa: E731
    assert _planes_group(lib, [chain(3 * 8192)], 3 * 8192, 3) == UNSUPPORTED          # L > 4096
    assert _planes_group(lib, [chain(5 * 4096)], 5 * 4096, 5) == UNSUPPORTED          # n > 16384
    assert _planes_group(lib, [chain(6 * 1024)], 6 * 1024, 6) == UNSUPPORTED          # K outside {3, 5, 7}
    assert _planes_group(lib, [chain(9 * 512)], 9 * 512, 9) == UNSUPPORTED
    # in_features == n, as for K == 1
    assert _planes_group(lib, [_chain_problem(p16, 5120, z_had=p16, had=p16, in_features=5000)], 5120, 5) == UNSUPPORTED
    # the fp16 group launch has no K > 1 chain
    arr = (capi.HadProblem * 1)(chain(5120))
    assert lib.quip_had_transform_group_f16(arr, 1, 1, 5120, 5, 1, None) == UNSUPPORTED
    # a launch is all chain or no chain
    plain = _chain_problem(p16, 5120, had=p16, z=None, x=p16)
    assert _planes_group(lib, [chain(5120), plain], 5120, 5) == UNSUPPORTED


def test_chain_alignment_and_aliasing_checks_hold_for_k_factors(lib, p16):
    n, K = 3584, 7
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=p16, had=p16, z=p16 + 2)], n, K) == MISALIGNED
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=p16, had=p16, h_out=p16 + 8)], n, K) == MISALIGNED
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=p16, had=p16, out=p16 + 4)], n, K) == MISALIGNED
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=p16, had=p16, h_out=p16 + 16)], n, K) == BAD_SHAPE   # == z_residual
    assert _planes_group(lib, [_chain_problem(p16, n, z_had=p16, had=p16, h_out=p16)], n, K) == BAD_SHAPE        # == z


def test_k1_chain_validation_is_unchanged(lib, p16):
    """K == 1 ignores z_had; its checks answer as before"""
    for z_had in (None, p16):
        assert _planes_group(lib, [_chain_problem(p16, 128, z_had=z_had)], 128, 1) == UNSUPPORTED        # L < 256
        assert _planes_group(lib, [_chain_problem(p16, 4096, z_had=z_had, in_features=4000)], 4096, 1) == UNSUPPORTED
        assert _planes_group(lib, [_chain_problem(p16, 4096, z_had=z_had, z_post_scale=None)], 4096, 1) == NULL_POINTER
        assert _planes_group(lib, [_chain_problem(p16, 4096, z_had=z_had, z=p16 + 2)], 4096, 1) == MISALIGNED
        assert _planes_group(lib, [_chain_problem(p16, 4096, z_had=z_had, h_out=p16 + 16)], 4096, 1) == BAD_SHAPE


@pytest.mark.parametrize("n,K", [(5120, 5), (3584, 7), (3072, 3)])
def test_fake_of_the_chain_op_with_k_factor(lib, n, K):
    t = lambda *s: torch.empty(*s, dtype=torch.float16, device="meta")   # noqa: E731
    z, vec, hk = t(1, n), t(n), t(K, K)
    for count in (1, 2, 3):
        for rs, m in ((0.0, n), (0.5, 2 * n), (register_lib.HI_PLANES, 2 * n)):
            out = torch.ops.quip_lib.had_chain_planes_group(z, vec, z, 1.0 / 32, n, [vec] * count, [1.0] * count, vec, 1e-5,
                                                            rs, K, hk, [hk] * count)
            assert len(out) == 1 + count
            assert out[0].shape == (1, n) and out[0].dtype == torch.float16 and out[0].device.type == "meta"
            for pl in out[1:]:
                assert pl.shape == (lib.quip_e8p_planes_bytes(m),) and pl.dtype == torch.uint8
    # the K == 1 call keeps its meaning
    out = torch.ops.quip_lib.had_chain_planes_group(t(1, 1024), t(1024), None, 1.0, 1024, [t(1024)], [1.0], None, 1e-5)
    assert out[0].shape == (1, 1024) and out[1].shape == (lib.quip_e8p_planes_bytes(1024),)


def _ql(fin, fout, use_rand=True, bias=False, per_channel=False):
    from quip_for_all_amd.decode import codebook_id
    from quip_for_all_amd.qlinear import QuantLinear
    cb = codebook_id["E8P12"](inference=True)
    return QuantLinear(fin, fout, cb, bias=bias, use_rand=use_rand, per_channel=per_channel).eval()


@pytest.mark.parametrize("hidden,K,L", [(5120, 5, 1024), (3584, 7, 512), (3072, 3, 1024)])
def test_chain_supported_for_k_factor_widths(hidden, K, L):
    from quip_for_all_amd.qlinear import chain_supported
    cons = [_ql(hidden, hidden), _ql(hidden, 512), _ql(hidden, 512)]
    prev = _ql(1024, hidden)
    assert all(l.K_left == K and l.q_in_features == K * L for l in cons) and prev.K_right == K
    assert chain_supported(cons, prev)
    assert chain_supported(cons[:1], prev)
    # the producer has to end in the same factorisation, plainly
    assert not chain_supported(cons, _ql(1024, 4096))                              # K_right == 1
    other = {5120: 3072, 3584: 5120, 3072: 3584}[hidden]
    assert not chain_supported(cons, _ql(1024, other))                             # another K, another width
    assert not chain_supported(cons, _ql(1024, hidden, bias=True))
    assert not chain_supported(cons, _ql(1024, hidden, per_channel=True))
    # consumers share one K
    assert not chain_supported([cons[0], _ql(4096, 512)], prev)


def test_chain_not_supported_for_the_table_factorisation_of_5120():
    """use_rand=False: 5120 = 20 x 256, a tall shape"""
    from quip_for_all_amd.qlinear import chain_supported
    cons = [_ql(5120, 512, use_rand=False)]
    prev = _ql(1024, 5120, use_rand=False)
    assert cons[0].K_left == 20 and prev.K_right == 20
    assert not chain_supported(cons, prev)
    assert not chain_supported(cons, _ql(1024, 5120))
    # and the power-of-two widths keep their answer
    assert chain_supported([_ql(4096, 4096), _ql(4096, 1024)], _ql(1024, 4096))


def test_python_shape_table_matches_the_librarys(lib, p16):
    """qlinear._chain_shape and fill() in csrc/hadamard.hip state the same (n, K) table: Python says yes exactly where
    the library's validation of a well-formed chain problem reaches the point of launching"""
    from quip_for_all_amd.qlinear import _chain_shape
    seen = 0
    for K in range(1, 12):
        for logL in range(6, 15):
            n = K << logL
            if n > 32768:
                continue
            # a device pointer the library refuses before it launches anything stands in for "would launch": rows of
            # planes must be 16-byte aligned, and that check comes after every shape check
            rc = _planes_group(lib, [_chain_problem(p16, n, z_had=p16, had=p16, out=p16 + 4)], n, K)
            assert rc in (MISALIGNED, UNSUPPORTED), (n, K, rc)
            assert _chain_shape(n, K) == (rc == MISALIGNED), (n, K, rc)
            seen += _chain_shape(n, K)
    assert seen == 7 + 4 + 3 + 3          # K = 1: 256..16384; K = 3: L 512..4096; K = 5, 7: L 512..2048 (n <= 16384)
