"""CPU-side pins of the two workspace layouts that hold reversed index lists (csrc/dvm_revlist.hip: RevListsT): the queries are
host code, and the layouts must stay what they were before the list builder was made one — a caller's buffer sized by an older
build must still fit."""
import pytest


def a(x):
    return (x + 255) // 256 * 256


@pytest.fixture(scope="module")
def lib():
    from dvm import _lib
    return _lib.load()


@pytest.mark.parametrize("B,N,K", [(1, 1, 1), (2, 1000, 40), (8, 2048, 40), (4, 12287, 8)])
def test_n2p_core_bwd_workspace_layout(lib, B, N, K):
    """de [B][N][K][4] floats | offs [B][N + 1] | cursor [B][N] | edges [B][N K] int2 | hist [B][64][N], each rounded up to 256."""
    need = a(16 * B * N * K) + a(4 * B * (N + 1)) + a(4 * B * N) + a(8 * B * N * K) + a(256 * B * N)
    assert lib.dvm_n2p_core_bwd_workspace_bytes(B, N, K) == need


@pytest.mark.parametrize("shape,nbytes", [((2, 300, 170, 10), 27136), ((8, 2048, 2048, 10), 786688)])
def test_apply_bwd_workspace_bytes(lib, shape, nbytes):
    """The literals are what dvm_softcorr_apply_bwd_workspace_bytes returned in a build of the commit before the list builder
    moved to dvm_revlist.hip (offs [B][M + 1] | cursor [B][M] | edges [B][N topk], each rounded up to 256)."""
    B, N, M, topk = shape
    assert nbytes == a(4 * B * (M + 1)) + a(4 * B * M) + a(4 * B * N * topk)
    assert lib.dvm_softcorr_apply_bwd_workspace_bytes(*shape) == nbytes
