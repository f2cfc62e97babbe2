"""MI355X checks of the row-table sampling kernel (``sample_rows_kernel`` in ``csrc/kernels/sample.hip``) against its
float64 twin (``ops.sample.sample_rows_reference``), against ``sample_logits``, on one-row slices, and of
``RequestSampler`` inside the continuous-batching decoder (eager and under the graph).  Kept counts, cuts, greedy
tokens and every state change are compared exactly; a sampled token's uniform must lie inside the twin's CDF interval
of that token within ``EPS = 1e-4``, the slack of ``tests/test_sample_gpu.py`` (same draw code, same bound)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from batch_decode_common import PROMPTS, make_model  # noqa: E402
from scaling_amd.ops.sample import sample_logits, sample_rows, sample_rows_reference, sample_uniform  # noqa: E402
from scaling_amd.transformer.inference import RequestSampler, SamplingParams as SP, sample_argmax  # noqa: E402

DEV = "cuda"
EPS = 1e-4
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _check_call(x, table, tokens, ref, info=None):
    """One call's tokens (and info) against the twin ``ref`` computed on the table as it was before the call."""
    kept, cdf, cut, _ = ref
    for b, tok in enumerate(tokens.tolist()):
        if int(table.active[b]) == 0:
            assert tok == 0
            continue
        if info is not None:
            assert info[b].tolist() == [int(kept[b].sum()), int(cut[b : b + 1].float().view(torch.int32))], b
        if not bool(kept[b].any()):
            assert tok == 0
        elif float(table.temperature[b]) == 0.0:
            assert tok == int(kept[b].to(torch.uint8).argmax()), b
        else:
            u = float(sample_uniform(int(table.seed[b]) & 0xFFFFFFFF, int(table.step[b]), 0))
            lo = float(cdf[b, tok - 1]) if tok > 0 else 0.0
            assert bool(kept[b, tok]) and lo - EPS <= u <= float(cdf[b, tok]) + EPS, (b, tok, lo, u, float(cdf[b, tok]))


def _copy(table):
    rs = RequestSampler(*table.hist.shape, DEV)
    rs.table.buf.copy_(table.buf)
    return rs.table


def _advanced(table, tokens):
    """The buffer of ``table`` after a call that returned ``tokens``: exactly the specified writes, on a copy."""
    t = _copy(table)
    for b, tok in enumerate(tokens.tolist()):
        if int(t.active[b]):
            n = int(t.hist_len[b])
            if n < t.hist.shape[1]:
                t.hist[b, n] = tok
                t.hist_len[b] = n + 1
            t.step[b] += 1
    return t.buf


def _logits(V, dtype):
    torch.manual_seed(V)
    base = ((torch.randn(7, V + 13, device=DEV) * 12).round() / 4).to(dtype)  # quarter steps: ties; negatives
    x = base[:, 3 : 3 + V]  # row stride V + 13, rows not 16-byte aligned
    if V > 3:
        x[2, 1] = float("-inf")
        x[3, 2] = float("nan")
        x[4, V - 1] = 2.5
    return x


def _rows(x, H=16):
    """The six rows of the issue plus row 6: both penalties under top-k and top-p, its history the row's twelve largest
    logits, so the cuts land among penalised values (full fp32 numbers, also where the logits are bf16 / fp16)."""
    V = x.shape[1]
    rs = RequestSampler(7, H, DEV)
    top = int(x[0].float().argmax())
    rs.set_row(0, SP(temperature=0.0, repetition_penalty=4.0, presence_penalty=1.0), [top])  # moves the argmax
    rs.set_row(1, SP(top_k=1, seed=11), [9] * 14)  # hist_len reaches H = 16 after two calls; no penalty
    rs.set_row(2, SP(temperature=0.7, top_k=40, top_p=0.9, seed=12))
    rs.set_row(3, SP(top_p=0.5, seed=13), [1])
    rs.set_row(4, SP(seed=14, repetition_penalty=1.3, presence_penalty=0.5), [5 % V, 5 % V, 0, V - 1, V + 3])
    rs.set_row(5, SP(temperature=0.3, seed=15, repetition_penalty=1.2), [0, 1])
    rs.clear_row(5)
    rs.set_row(6, SP(0.7, 8, 0.9, seed=16, repetition_penalty=1.3, presence_penalty=0.5),
               x[6].float().topk(min(12, V)).indices.tolist())
    return rs


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("V", [1, 69, 1000, 32768, 32769])
def test_kernel_matches_twin(V, dtype):
    x = _logits(V, DTYPES[dtype])
    rs = _rows(x)
    t = rs.table
    if V > 3:
        pen = sample_rows_reference(x, t)[3]
        assert int(pen[0].argmax()) != int(x[0].float().argmax())  # the penalty changes the greedy token
    drawn = None
    for call in range(3):
        ref, was = sample_rows_reference(x, t), _copy(t)  # the table as it is before the call
        if drawn is not None:  # the token row 4 drew in the previous call is penalised in this one
            assert float(ref[3][4, drawn]) < float(x[4, drawn])
        tokens, info = sample_rows(x, t, want_info=torch.full((7, 2), -7, dtype=torch.int32, device=DEV))
        _check_call(x, was, tokens, ref, info)
        assert torch.equal(t.buf, _advanced(was, tokens)), call  # every row, the parked one bytewise unchanged
        assert info[5].tolist() == [-7, -7] and int(tokens[5]) == 0
        drawn = int(tokens[4])
    assert int(was.hist_len[1]) == 16 and int(t.hist_len[1]) == 16 and int(t.step[1]) == 3  # full: drawn, not appended


@pytest.mark.parametrize("V", [1000, 32769])
def test_agrees_with_sample_logits(V):
    """Penalties off, equal parameters in every row: info is ``sample_logits``'s bit for bit, and row 0's token is
    ``sample_logits``'s for the same (seed, step) -- its row term is 0 there too."""
    x = _logits(V, torch.bfloat16)
    rs = RequestSampler(7, 8, DEV)
    for b in range(7):
        rs.set_row(b, SP(0.8, 40, 0.95, seed=3), [1, 2])
    for step in range(3):
        tokens, info = sample_rows(x, rs.table, want_info=True)
        want, winfo = sample_logits(x, step, 3, 0.8, 40, 0.95, want_info=True)
        assert torch.equal(info, winfo) and int(tokens[0]) == int(want[0])


@pytest.mark.parametrize("r", [0, 2, 6])
def test_one_row_slice(r):
    x = _logits(1000, torch.bfloat16)
    whole, part = _rows(x), _rows(x)
    tokens = sample_rows(x, whole.table)
    before = part.table.buf.clone()
    tok = sample_rows(x[r : r + 1], part.table.rows(r, r + 1))
    assert tok.tolist() == [int(tokens[r])]
    before[r] = whole.table.buf[r]
    assert torch.equal(part.table.buf, before)  # row r changed as in the full call, no other row touched


@pytest.fixture(scope="module")
def model():
    return make_model(0, "bfloat16")


PARAMS = [SP(0.8, 40, 0.95, seed=1), SP(0.0, repetition_penalty=1.3), SP(1.0, 20, 0.9, seed=2, repetition_penalty=1.3,
          presence_penalty=0.5), SP(0.7, top_p=0.9, seed=3, penalize_prompt=False), SP(1.2, 20, seed=4)]
LIMITS = [30, 6, 12, 20, 9]


def _serve(model, order, graph):
    dec = model.continuous_decoder(4, page_size=32, max_pages=3, skinny_gemm=True, use_cuda_graph=graph, sampling=True)
    out = dec.serve([(PROMPTS[i], LIMITS[i]) for i in order], [], sampling=[PARAMS[i] for i in order])
    assert dec.captures == (1 if graph else 0) and dec.free_rows == [0, 1, 2, 3]
    assert not bool(dec.sample_fn.table.active.any())
    return {i: (t, lg.clone()) for i, (t, lg) in zip(order, out)}


def test_decoder_per_request_sampling(model):
    eager, graph = _serve(model, [0, 1, 2, 3, 4], False), _serve(model, [0, 1, 2, 3, 4], True)
    for i in range(5):
        assert graph[i][0] == eager[i][0] and len(graph[i][0]) == LIMITS[i], i
        # the request alone against the twin: its recorded logits, its own running history and draw counter
        rs = RequestSampler(1, 96, DEV)
        rs.set_row(0, PARAMS[i], PROMPTS[i])
        for tok, lg in zip(*graph[i]):
            x = lg[None]
            _check_call(x, rs.table, torch.tensor([tok]), sample_rows_reference(x, rs.table))
            rs.table.buf.copy_(_advanced(rs.table, torch.tensor([tok])))
    # placement: request 0 in row 0 from the start, or in row 2 after request 1 (6 tokens) has left it
    moved = _serve(model, [3, 2, 1, 4, 0], True)
    assert torch.equal(moved[0][1], graph[0][1])  # rows of the skinny / attention / append kernels are independent
    assert moved[0][0] == graph[0][0]
    # a greedy request without penalties is sample_argmax on its recorded logits
    plain = model.continuous_decoder(4, page_size=32, max_pages=3, skinny_gemm=True, use_cuda_graph=True, sampling=True)
    (tokens, logits), = plain.serve([(PROMPTS[0], 10)], [], sampling=SP(0.0))
    assert tokens == [int(sample_argmax(lg[None, None])) for lg in logits]
