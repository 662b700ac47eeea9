"""The shared layer under the frozen-feature evaluators (contrad_amd/features.py) on the GPU: the one row-chunk loop that
kNN, PRDC and KID run through, the banks, and the feature extraction, at the smallest shapes where they can go wrong
(70 query rows in chunks of 16: four full chunks and one of 6; a bank of 301 rows: three zero padding columns; 10 images
in batches of 4: a partial last batch).

The similarities of L2-normalised fp32 rows are held against the float64 product of the same fp32 rows with the bound of
tests/test_knn_gpu.py, (2 d + 8) * 2^-24 (its docstring derives it; the dot product alone needs d * 2^-24 of it)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
M, N, D_FEAT, CHUNK = 70, 301, 24, 16
N_PAD = 304
_STATE = {}


def _rows():
    """(q [70, 24], bank rows [301, 24], the transposed bank [24][304]): normalised device rows, made once."""
    if not _STATE:
        from contrad_amd import features
        g = torch.Generator(device='cpu').manual_seed(0)
        q = features.normalize_rows(torch.randn(M, D_FEAT, generator=g).cuda())
        rows = features.normalize_rows(torch.randn(N, D_FEAT, generator=g).cuda())
        _STATE['rows'] = (q, rows, features.bank_of(rows))
    return _STATE['rows']


def _bits(t):
    return t.contiguous().view(torch.int32)


def _chunks(**how):
    from contrad_amd import features
    q, _, bankT = _rows()
    return [(i, S.clone()) for i, S in features.similarity_chunks(q, bankT, **how)]


def test_chunks_partition_the_rows_and_equal_the_direct_gemm(margin):
    from contrad_amd import features
    q, rows, bankT = _rows()
    assert tuple(bankT.shape) == (D_FEAT, N_PAD)
    chunks = _chunks(chunk_rows=CHUNK)
    assert [i for i, _ in chunks] == [0, 16, 32, 48, 64] and [S.shape[0] for _, S in chunks] == [16, 16, 16, 16, 6]
    for i, S in chunks:
        assert tuple(S.shape) == (min(CHUNK, M - i), N_PAD) and S.dtype == torch.float32
        direct = features.similarities(q[i:i + S.shape[0]], bankT, torch.empty(S.shape[0], N_PAD, device='cuda'))
        assert torch.equal(_bits(S), _bits(direct)), i
        assert bool((S[:, N:] == 0).all()), i                         # the padding columns [301, 304)
    whole = torch.cat([S for _, S in chunks])
    ref = q.cpu().double().numpy() @ rows.cpu().double().numpy().T      # float64 product of the same fp32 rows
    margin('features similarity chunks 70x301x24', np.abs(whole[:, :N].cpu().numpy().astype(np.float64) - ref).max(),
           (2 * D_FEAT + 8) * EPS)


def test_the_chunk_size_is_read_from_the_module_at_call_time(monkeypatch):
    from contrad_amd import features
    given = _chunks(chunk_rows=CHUNK)
    assert [i for i, _ in _chunks()] == [0]                           # the default rule: 70 rows are one chunk
    monkeypatch.setattr(features, 'MAX_CHUNK_ROWS', CHUNK)
    assert features.chunk_rows_of(N_PAD) == CHUNK
    patched = _chunks()
    assert [i for i, _ in patched] == [i for i, _ in given]
    for (_, a), (_, b) in zip(patched, given):
        assert torch.equal(_bits(a), _bits(b))


def test_a_callers_buffer_is_the_only_S():
    from contrad_amd import features
    q, _, bankT = _rows()
    given = _chunks(chunk_rows=CHUNK)                                 # (also: first-use allocations of the GEMM are made)
    S = torch.empty(CHUNK, N_PAD, device='cuda')
    lo, hi = S.data_ptr(), S.data_ptr() + S.numel() * 4
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    seen = []
    for (i, Sc), (j, ref) in zip(features.similarity_chunks(q, bankT, S), given):
        assert i == j and lo <= Sc.data_ptr() and Sc.data_ptr() + Sc.numel() * 4 <= hi and Sc.is_contiguous()
        seen.append(torch.cuda.max_memory_allocated() - base)
        assert torch.equal(_bits(Sc), _bits(ref))
    assert len(seen) == 5 and max(seen) < S.numel() * 4, seen         # nothing of a chunk's size was allocated besides


def test_zero_rows_yield_nothing():
    from contrad_amd import features, knn
    q, rows, bankT = _rows()
    assert list(features.similarity_chunks(q[:0], bankT)) == []
    assert list(features.similarity_chunks(q[:0], bankT, torch.empty(CHUNK, N_PAD, device='cuda'))) == []
    assert list(features.similarity_chunks(q[:0], bankT, chunk_rows=CHUNK)) == []
    clf = knn.KNNClassifier(rows, np.arange(N) % 5, 5, k=7, temp=0.1, normalize=False)      # (the rows are normalised already)
    pred, scores, idx, val = clf.predict(q[:0], neighbours=True)
    assert (tuple(pred.shape), pred.dtype) == ((0,), torch.int32) and (tuple(scores.shape), scores.dtype) == ((0, 5), torch.float32)
    assert (tuple(idx.shape), idx.dtype) == ((0, 7), torch.int32) and (tuple(val.shape), val.dtype) == ((0, 7), torch.float32)
    assert len(clf.predict(q[:0])) == 2


def test_banks_by_rows_and_by_columns_hold_the_same_bytes():
    from contrad_amd import features
    _, rows, bankT = _rows()
    by_columns = features.new_bank(N, D_FEAT, rows.device)
    assert tuple(by_columns.shape) == (D_FEAT, N_PAD) and not bool(by_columns.any())
    for i in range(0, N, 100):                                        # column copies, as extract_features writes a bank
        m = min(100, N - i)
        by_columns[:, i:i + m].copy_(rows[i:i + m].t())
    assert torch.equal(_bits(by_columns), _bits(bankT)) and bool((bankT[:, N:] == 0).all())


def test_extract_features_into_a_bank_gives_the_same_floats():
    from contrad_amd import features
    from contrad_amd.evaluate.gan import freeze
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(3)
    D = freeze(get_architecture('sndcgan', (32, 32, 3))[1].cuda())
    x = torch.randint(0, 256, (10, 32, 32, 3), generator=torch.Generator().manual_seed(1)).to(torch.uint8).cuda()
    rows = features.extract_features(D, x, 4)                         # batches of 4, 4 and 2
    assert tuple(rows.shape) == (10, D.d_penul)
    bank = features.new_bank(10, D.d_penul, x.device)
    assert features.extract_features(D, x, 4, bankT=bank) is bank and tuple(bank.shape) == (D.d_penul, 12)
    assert torch.equal(_bits(bank[:, :10].t()), _bits(rows)) and not bool(bank[:, 10:].any())
