"""The one rule for blocks derived from weights (kernels.weights_key / kernels.cached_block) on its three users: VASNet, the
Transformer scorer and the BiLSTM scorers keep the bf16 planes of their weight matrices in model._wpl."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(kind, dev):
    """(model, packed features, lens, first block of model._wpl) at the smallest shape on the plane path: the narrowest weights with a
    non-zero sumk_*_wplanes_bytes (D = 256; BiLSTM: In = 128, 8H = 256) and two videos that just pass the row gate of the Python layer
    (256 rows; BiLSTM: 1024)."""
    torch.manual_seed(5)
    if kind == "vasnet":
        from summarizer_amd.models.vasnet import VASNet
        m, D, lens = VASNet(input_size=256, precision="bf16x6"), 256, [130, 126]
    elif kind == "transformer":
        from summarizer_amd.models.transformer import Transformer
        m, D, lens = Transformer(input_size=256, encoder_layers=1, attention_heads=4), 256, [130, 126]
    else:
        from summarizer_amd.models.dsn import DSN
        m, D, lens = DSN(input_size=128, hidden_size=32), 128, [513, 511]
    m.precision = "bf16x6"
    x = (torch.randn(sum(lens), D) * 0.1).to(dev)
    return m.to(dev).eval(), x, lens, (lambda: m._wpl[0]) if kind == "bilstm" else (lambda: m._wpl)


@pytest.mark.parametrize("kind", ["vasnet", "transformer", "bilstm"])
def test_weight_planes_are_cached_per_weights_and_stream(dev, kind):
    """A second call re-uses the block; an optimiser step through the C ABI (FlatAdam.step: torch sees neither a new address nor a new
    tensor version, only kernels.WEIGHTS_EPOCH moves) changes the key and the scores; a call on another stream gets a block in a
    backing buffer of its own (kernels the default stream has queued may still read the old one) and the same scores."""
    from summarizer_amd import _lib, kernels
    from summarizer_amd.training import FlatAdam
    m, x, lens, block = _model(kind, dev)
    opt = FlatAdam(m.parameters(), lr=1e-2)          # (first: it moves the weights into its flat bucket, a change of address)

    def score():
        with torch.no_grad():
            return m.score_packed(x, lens)
    s0 = score()
    # the plane path ran (tests/test_gpu_planes.py, tests/test_gpu_transformer.py)
    assert block() is not None
    if kind == "transformer":          # (the encoder splits its layer inputs itself: the batch qualifies when the plane path's workspace applies)
        lib, sb = _lib.load(), kernels.SeqBatch.get(lens, dev)
        args = (256, 256, 4, 1, sb.n_seq, sb.off_host_p, 0)
        assert lib.sumk_transformer_workspace_bytes_for(*args, kernels.precision_code("bf16x6")) > lib.sumk_transformer_workspace_bytes(*args)
    else:
        assert "planes3" in x._sumk_shadows
    key0, ptr0 = m._wpl_key, block().data_ptr()
    assert torch.equal(score(), s0) and m._wpl_key == key0 and block().data_ptr() == ptr0          # re-used

    seen = [(p.data_ptr(), p._version) for p in m.parameters()]
    epoch = kernels.WEIGHTS_EPOCH[0]
    opt.zero_grad()
    opt.flat_grad.fill_(0.01)
    opt.step()
    assert [(p.data_ptr(), p._version) for p in m.parameters()] == seen and kernels.WEIGHTS_EPOCH[0] > epoch
    s1 = score()
    key1 = m._wpl_key
    assert key1 != key0 and not torch.equal(s1, s0)

    buf = block()._sumk_keep          # (held: the allocator cannot hand its address to the side stream's buffer)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        s2 = score()
    side.synchronize(); torch.cuda.current_stream(dev).synchronize()
    assert m._wpl_key[:-1] == key1[:-1] and m._wpl_key[-1] != key1[-1]          # the same weights, another stream
    assert block()._sumk_keep is not buf and block()._sumk_keep.data_ptr() != buf.data_ptr()
    assert torch.equal(s2, s1)
    kernels.health_check()
