"""``text_mask_words_kernel`` against its emulation (bit-exact), against ``text_mask`` with an
all-zero table, under graph replay, and through ``PerceiverMLM.loss`` on the fused path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
V, UNK, MASK, LO, P = 10003, 1, 2, 3, 0.15
STATE = [0x123456789AB, 5, 0]


def _ext():
    from perceiver_io_amd.ops import ext

    return ext.require()


def _emu():
    from perceiver_io_amd.ops import emulation

    return emulation


@pytest.fixture(scope="module")
def table():
    from perceiver_io_amd.data.imdb import shipped_tokenizer
    from perceiver_io_amd.utils.tokenizer import continuation_table

    return continuation_table(shipped_tokenizer(V))


@pytest.fixture(scope="module")
def packed(table):
    from perceiver_io_amd.utils.tokenizer import pack_bits

    return pack_bits(table).to(DEV)


def _batch(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, V, shape, generator=g)
    pad = torch.rand(shape, generator=g) < 0.2
    return x.to(DEV), pad.to(DEV)


def _launches(x, pad, packed, vocab=V):
    """three advancing launches and one that does not advance: outputs and state equal the emulation's"""
    st_k = torch.tensor(STATE, device=DEV)
    st_e = st_k.clone()
    seen = []
    for advance in (True, True, True, False):
        a = _ext().text_mask_words(x, pad, st_k, packed, UNK, MASK, P, LO, vocab, advance)
        b = _emu().text_mask_words(x, pad, st_e, packed, UNK, MASK, P, LO, vocab, advance)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(st_k, st_e) and int(st_k[2]) == 0
        seen.append(a[1])
    assert int(st_k[1]) == STATE[1] + 3
    if x.numel() >= 1000:  # fresh masks on every advancing launch
        assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    return seen


@pytest.mark.parametrize("with_pad", [False, True])
@pytest.mark.parametrize("shape", [(1, 1), (5, 37), (3, 300), (2, 1024)])
def test_kernel_matches_emulation(shape, with_pad, packed):
    x, pad = _batch(shape, seed=shape[1])
    _launches(x, pad if with_pad else None, packed)


@pytest.mark.parametrize("with_pad", [False, True])
def test_planted_words(with_pad, table, packed):
    """Words across a wave boundary (62–66) and a tile boundary (254–258), a word ending at a row's
    last column before a continuation at column 0, a 40-token continuation run, an
    all-continuation row, ids −1 and V, and a special token inside a word."""
    cont = table.nonzero().squeeze(1)
    plain = (~table).nonzero().squeeze(1)
    plain = plain[plain >= LO]
    g = torch.Generator().manual_seed(5)
    B, L = 4, 300
    x = plain[torch.randint(0, plain.numel(), (B, L), generator=g)]
    c = lambda n: cont[torch.randint(0, cont.numel(), (n,), generator=g)]  # noqa: E731
    x[0, 63:67] = c(4)      # word 62–66
    x[0, 255:259] = c(4)    # word 254–258
    x[0, 297:300] = c(3)    # word 296–299 ends the row
    x[1, 0:2] = c(2)        # continuation at column 0: a word of its own
    x[1, 10:50] = c(40)     # 41-token word: the tail past 16 tokens goes token by token
    x[1, 100:110] = c(10)
    x[1, 104] = -1
    x[1, 107] = V
    x[1, 120:126] = c(6)
    x[1, 123] = UNK
    x[2, :] = c(L)          # all continuations
    x = x.to(DEV)
    pad = None
    if with_pad:
        pad = torch.zeros(B, L, dtype=torch.bool)
        pad[0, 64] = pad[2, 77] = pad[3, 250:] = True
        pad = pad.to(DEV)
    seen = _launches(x, pad, packed)
    if not with_pad:  # every launch takes or leaves the planted words whole
        for lab in seen:
            sel = (lab != -100).cpu()
            for row, a, b in ((0, 62, 67), (0, 254, 259), (0, 296, 300), (1, 0, 2), (1, 9, 25), (2, 0, 16), (2, 16, 17)):
                assert sel[row, a:b].all() or not sel[row, a:b].any(), (row, a, b)
    _ext().check_errors(True)  # a checked build records the two ids outside the table


def test_grid_stride_tiles(packed):
    """more tokens than the capped grid covers in one pass: every workgroup walks several tiles"""
    x, pad = _batch((1100, 1024), seed=11)
    assert x.numel() > 4096 * 256
    st_k = torch.tensor(STATE, device=DEV)
    st_e = st_k.clone()
    a = _ext().text_mask_words(x, pad, st_k, packed, UNK, MASK, P, LO, V, True)
    b = _emu().text_mask_words(x, pad, st_e, packed, UNK, MASK, P, LO, V, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(st_k, st_e)


@pytest.mark.parametrize("shape", [(5, 37), (3, 300), (64, 512)])
def test_zero_table_equals_text_mask(shape):
    x, pad = _batch(shape, seed=2)
    zero = torch.zeros((V + 31) // 32, dtype=torch.int32, device=DEV)
    st_w = torch.tensor(STATE, device=DEV)
    st_t = st_w.clone()
    for advance in (True, False):
        a = _ext().text_mask_words(x, pad, st_w, zero, UNK, MASK, P, LO, V, advance)
        b = _ext().text_mask(x, pad, st_t, UNK, MASK, P, LO, V, advance)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(st_w, st_t)


def test_binding_checks(packed):
    x, pad = _batch((3, 40))
    st = torch.tensor(STATE, device=DEV)
    K = _ext()
    with pytest.raises(RuntimeError):
        K.text_mask_words(x.reshape(-1), None, st, packed, UNK, MASK, P, LO, V, False)  # not (B, L)
    with pytest.raises(RuntimeError):
        K.text_mask_words(x, pad, st, packed[:-1].contiguous(), UNK, MASK, P, LO, V, False)  # short table
    with pytest.raises(RuntimeError):
        K.text_mask_words(x, pad, st, packed.to(torch.int64), UNK, MASK, P, LO, V, False)  # dtype
    with pytest.raises(RuntimeError):
        K.text_mask_words(x, pad, st, packed.cpu(), UNK, MASK, P, LO, V, False)  # device
    assert st.tolist() == STATE


def test_graph_replay_draws_fresh_masks(packed):
    x, pad = _batch((3, 300), seed=3)
    st_k = torch.tensor(STATE, device=DEV)
    st_e = st_k.clone()
    K = _ext()
    K.text_mask_words(x, pad, st_k, packed, UNK, MASK, P, LO, V, True)  # eager: the state exists before capture
    _emu().text_mask_words(x, pad, st_e, packed, UNK, MASK, P, LO, V, True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = K.text_mask_words(x, pad, st_k, packed, UNK, MASK, P, LO, V, True)
    last = None
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        want = _emu().text_mask_words(x, pad, st_e, packed, UNK, MASK, P, LO, V, True)
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
        assert torch.equal(st_k, st_e)
        assert last is None or not torch.equal(last, out[1])
        last = out[1].clone()
    assert st_k.tolist() == [STATE[0], STATE[1] + 4, 0]


def test_mlm_loss_with_whole_word_masking_on_the_fused_path():
    """``PerceiverMLM.loss`` drawing whole-word masks in the kernel equals the loss replayed with
    the emulation's masks from the same state (shape and tolerance of ``test_model_gpu``'s fused vs
    emulation MLM loss); nothing overflows the selection capacity."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.models import TextMasking
    from perceiver_io_amd.tasks import LitMaskedLanguageModel
    from perceiver_io_amd.utils.tokenizer import pack_bits

    torch.manual_seed(0)
    vocab, L, B = 500, 96, 6
    lit = LitMaskedLanguageModel(vocab_size=vocab, max_seq_len=L,
                                 optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                                 num_latents=64, num_latent_channels=64, num_encoder_layers=2,
                                 num_encoder_self_attention_layers_per_block=2)
    cont = torch.rand(vocab) < 0.3
    cont[:LO] = False
    lit.model.masking = TextMasking(vocab, whole_word=True, continuation=cont, word_clump=2.0)
    m = lit.cuda().model
    ids = torch.randint(LO, vocab, (B, L), device=DEV)
    pad = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    pad[B // 2, 2 * L // 3:] = True
    st = ops.masking.mask_state(ids.device)
    st.copy_(torch.tensor(STATE))
    st0 = st.clone()
    ops.mlm_head.check_overflow(reset=True)
    with ops.backend("hip"):
        l_fused = m.loss(ids, pad)
    xm, lab = _emu().text_mask_words(ids, pad, st0, pack_bits(cont).to(DEV), UNK, MASK, P, LO, vocab, True)
    assert torch.equal(st, st0)
    assert (lab != -100).sum() > 0
    with ops.backend("hip"):
        l_replay = m.loss(ids, pad, labels=lab, x_masked=xm)
    assert abs(l_fused.item() - l_replay.item()) < 1e-3 * abs(l_replay.item()), (l_fused.item(), l_replay.item())
    assert ops.mlm_head.check_overflow(reset=True) is False
