"""Whole-word masking on the CPU: the emulation of ``text_mask_words_kernel`` against the token-level
masking (all-zero table), against word heads from a plain Python loop, its selection statistics and
the capacity they need, the tokenizer helpers, and the ``mlm`` command line with the flag on."""
import math
import os

import pytest
import torch

from perceiver_io_amd.data.imdb import shipped_tokenizer
from perceiver_io_amd.ops import emulation
from perceiver_io_amd.ops.mlm_head import capacity, row_capacity
from perceiver_io_amd.utils.tokenizer import continuation_table, pack_bits, word_clump

TOKENIZER = shipped_tokenizer(10003)
V, UNK, MASK, LO, P, W = 10003, 1, 2, 3, 0.15, 16
SHAPES = [(5, 37), (3, 300), (64, 512)]
STATE = [0x123456789AB, 5, 0]


@pytest.fixture(scope="module")
def table():
    return continuation_table(TOKENIZER)


def _batch(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, V, shape, generator=g)
    pad = torch.rand(shape, generator=g) < 0.2
    return x, pad


def py_heads(x, pad, table, unk=UNK, window=W):
    """Word heads (flat indices) by the rules of the issue, token by token in plain Python."""
    B, L = x.shape
    xs, ps, tb = x.tolist(), (pad.tolist() if pad is not None else None), table.tolist()

    def special(b, c):
        return xs[b][c] == unk or (ps is not None and ps[b][c])

    def cont(t):
        return tb[t] if 0 <= t < len(tb) else False

    def begins(b, c):
        return c == 0 or special(b, c) or special(b, c - 1) or not cont(xs[b][c])

    heads = []
    for b in range(B):
        row = []
        for c in range(L):
            h = c
            for k in range(window):
                if c - k < 0:
                    break
                if begins(b, c - k):
                    h = c - k
                    break
            else:
                h = c
            row.append(b * L + h)
        heads.append(row)
    return torch.tensor(heads)


def _special(x, pad):
    return (x == UNK) | pad if pad is not None else x == UNK


@pytest.mark.parametrize("shape", SHAPES)
def test_zero_table_is_token_level_masking(shape):
    x, pad = _batch(shape)
    zero = torch.zeros((V + 31) // 32, dtype=torch.int32)
    sa, sb = torch.tensor(STATE), torch.tensor(STATE)
    for advance in (True, True, False):
        a = emulation.text_mask_words(x, pad, sa, zero, UNK, MASK, P, LO, V, advance)
        b = emulation.text_mask(x, pad, sb, UNK, MASK, P, LO, V, advance)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert torch.equal(sa, sb)
    assert sa.tolist() == [STATE[0], STATE[1] + 2, 0]


@pytest.mark.parametrize("shape", SHAPES)
def test_words_are_selected_whole_and_at_rate_p(shape, table):
    x, pad = _batch(shape, seed=1)
    xm, labels = emulation.text_mask_words(x, pad, torch.tensor(STATE), pack_bits(table), UNK, MASK, P, LO, V, True)
    special = _special(x, pad)
    heads = py_heads(x, pad, table)
    sel = labels != -100
    assert not sel[special].any()
    ns = ~special
    assert torch.equal(sel[ns], sel.reshape(-1)[heads][ns])  # a token is selected iff its word's first token is
    assert torch.equal(labels[sel], x[sel]) and torch.equal(xm[~sel], x[~sel])
    assert (heads != torch.arange(x.numel()).view(shape))[ns].any()  # the batch has multi-token words
    # the count of selected tokens: mean p·n, variance p(1 − p)·Σ len² = p(1 − p)·r·n
    n, count = int(ns.sum()), int(sel.sum())
    r = word_clump(x, pad, table, UNK)
    assert 1.0 < r < 3.0
    z = (count - P * n) / math.sqrt(P * (1 - P) * r * n)
    print(f"{shape}: n {n} selected {count} clump {r:.3f} z {z:+.2f} max per row {int(sel.sum(1).max())}")
    assert abs(count - P * n) <= 6 * math.sqrt(P * (1 - P) * r * n)
    assert int(sel.sum(1).max()) <= row_capacity(shape[1], P, 1.0)


def test_word_clump_is_sum_len2_over_sum_len(table):
    x, pad = _batch((3, 300), seed=2)
    heads = py_heads(x, pad, table)
    ns = ~_special(x, pad)
    lens = {}
    for h in heads[ns].tolist():
        lens[h] = lens.get(h, 0) + 1
    want = sum(v * v for v in lens.values()) / sum(lens.values())
    assert word_clump(x, pad, table, UNK) == pytest.approx(want, rel=1e-12)
    assert word_clump(x, pad, torch.zeros_like(table), UNK) == 1.0
    assert word_clump(torch.full((2, 4), UNK), None, table, UNK) == 1.0


def test_capacity_clump():
    for L in (37, 300, 512, 2048):
        assert row_capacity(L, P, 1.0) == row_capacity(L, P)
        assert capacity(64 * L, P, 1.0) == capacity(64 * L, P)
        caps = [row_capacity(L, P, c) for c in (1.0, 1.5, 2.0, 3.0, 8.0)]
        gcaps = [capacity(64 * L, P, c) for c in (1.0, 1.5, 2.0, 3.0, 8.0)]
        assert caps == sorted(caps) and gcaps == sorted(gcaps)
    assert row_capacity(512, P) == 160 and row_capacity(512, P, 2.0) > 160
    assert capacity(64 * 512, P, 2.0) > capacity(64 * 512, P)


def _edge_rows(table):
    cont = table.nonzero().squeeze(1)[:64].tolist()
    plain = (~table).nonzero().squeeze(1)
    plain = plain[plain >= LO][:64].tolist()
    return cont, plain


def test_edges_against_the_python_loop(table):
    cont, plain = _edge_rows(table)
    L = 64
    rows = []
    # 0: ends in a word's first piece + continuation at the last column
    rows.append([plain[i % 7] for i in range(L - 2)] + [plain[0], cont[0]])
    # 1: begins with a continuation: its own word, not the tail of row 0's last word
    rows.append([cont[1], cont[2]] + [plain[i % 5] for i in range(L - 2)])
    # 2: continuations after a pad (column 3) and after UNK (column 10)
    r = [plain[i % 9] for i in range(L)]
    r[4], r[5], r[10], r[11], r[12] = cont[3], cont[4], UNK, cont[5], cont[6]
    rows.append(r)
    # 3: a 40-token all-continuation run after one plain token
    rows.append([plain[1]] + [cont[i % 11] for i in range(40)] + [plain[i % 3] for i in range(L - 41)])
    # 4: ids −1 and V between continuations
    r = [plain[2]] + [cont[i % 13] for i in range(L - 1)]
    r[7], r[20] = -1, V
    rows.append(r)
    x = torch.tensor(rows)
    pad = torch.zeros_like(x, dtype=torch.bool)
    pad[2, 3] = True
    heads = py_heads(x, pad, table)
    flat = lambda b, c: b * L + c  # noqa: E731
    # the rules, spelt out
    assert heads[0, L - 1] == flat(0, L - 2)
    assert heads[1, 0] == flat(1, 0) and heads[1, 1] == flat(1, 0)
    assert heads[2, 4] == flat(2, 4) and heads[2, 5] == flat(2, 4)  # after the pad: begins its own word
    assert heads[2, 11] == flat(2, 11) and heads[2, 12] == flat(2, 11)  # after UNK
    assert heads[3, 15] == flat(3, 0) and heads[3, 16] == flat(3, 16) and heads[3, 40] == flat(3, 40)
    assert heads[4, 7] == flat(4, 7) and heads[4, 8] == flat(4, 7) and heads[4, 20] == flat(4, 20)
    special = _special(x, pad)
    assert torch.equal(emulation.word_heads(special, emulation.unpack_bits(pack_bits(table), x, V)), heads)
    # the masks follow the heads under several counters; tokens after a pad / UNK are selectable
    packed = pack_bits(table)
    state = torch.tensor(STATE)
    picked = torch.zeros_like(special)
    for _ in range(40):
        _, labels = emulation.text_mask_words(x, pad, state, packed, UNK, MASK, P, LO, V, True)
        sel = labels != -100
        assert not sel[special].any()
        assert torch.equal(sel[~special], sel.reshape(-1)[heads][~special])
        picked |= sel
    assert picked[2, 4] and picked[2, 11] and picked[1, 0] and picked[4, 7] and picked[4, 20]


def test_continuation_table_of_the_shipped_tokenizer(table):
    import json

    from perceiver_io_amd.utils.tokenizer import load_tokenizer

    vocab = json.load(open(TOKENIZER, encoding="utf-8"))["model"]["vocab"]
    assert table.dtype == torch.bool and table.shape == (V,)
    assert int(table.sum()) == 2051
    by_id = {i: t for t, i in vocab.items()}
    assert all(by_id[i].startswith("##") for i in table.nonzero().squeeze(1).tolist())
    assert not table[:LO].any()
    assert torch.equal(continuation_table(load_tokenizer(TOKENIZER)), table)
    packed = pack_bits(table)
    assert packed.dtype == torch.int32 and packed.shape == ((V + 31) // 32,)
    ids = torch.arange(-2, V + 40)
    want = torch.zeros(ids.shape, dtype=torch.bool)
    want[2:V + 2] = table
    assert torch.equal(emulation.unpack_bits(packed, ids, V), want)


def test_text_masking_module(table):
    from perceiver_io_amd import ops
    from perceiver_io_amd.models import TextMasking
    from perceiver_io_amd.utils.tokenizer import load_tokenizer

    with pytest.raises(ValueError, match="continuation"):
        TextMasking(V, whole_word=True)
    with pytest.raises(ValueError, match="entries"):
        TextMasking(V + 1, whole_word=True, continuation=table)
    plain = TextMasking(V)
    ww = TextMasking.create(load_tokenizer(TOKENIZER), whole_word=True, word_clump=1.7)
    assert ww.whole_word and ww.word_clump == 1.7 and plain.word_clump == 1.0
    assert TextMasking(V, word_clump=3.0).word_clump == 1.0  # used only with whole-word masking
    assert torch.equal(ww.word_table, pack_bits(table)) and plain.word_table is None
    assert list(ww.state_dict()) == list(plain.state_dict())
    x, pad = _batch((5, 37), seed=3)
    ops.masking.reset_mask_state()
    st = ops.masking.mask_state("cpu").clone()
    got = ww(x, pad)
    want = emulation.text_mask_words(x, pad, st, pack_bits(table), UNK, MASK, P, LO, V, True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(ops.masking.mask_state("cpu"), st)
    with ops.backend("reference"), pytest.raises(RuntimeError, match="whole-word"):
        ww(x, pad)
    ops.masking.reset_mask_state()


def test_loss_has_room_for_whole_word_selection(table):
    """The (64, 512) batch through ``PerceiverMLM.loss`` with whole-word masking: no selected
    position falls out of the fixed capacity."""
    from perceiver_io_amd import ops
    from perceiver_io_amd.tasks import LitMaskedLanguageModel

    torch.manual_seed(0)
    lit = LitMaskedLanguageModel(vocab_size=V, max_seq_len=512, whole_word_masking=True,
                                 optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
                                 num_latents=8, num_latent_channels=16, num_encoder_layers=1,
                                 num_encoder_self_attention_layers_per_block=1, num_encoder_cross_attention_heads=1,
                                 num_encoder_self_attention_heads=1, num_decoder_cross_attention_heads=1)
    m = lit.model
    assert m.masking.whole_word and m.masking.word_clump == 2.0 and m.masking.mask_p == 0.15
    x, pad = _batch((64, 512), seed=1)
    ops.mlm_head.check_overflow(reset=True)
    with torch.no_grad():
        loss = m.loss(x, pad)
    assert torch.isfinite(loss)
    assert ops.mlm_head.check_overflow(reset=True) is False


def test_task_options_and_table_size():
    from perceiver_io_amd.tasks import LitMaskedLanguageModel

    kw = dict(max_seq_len=32, optimizer_init={"class_path": "torch.optim.AdamW", "init_args": {"lr": 1e-3}},
              num_latents=4, num_latent_channels=16, num_encoder_layers=1,
              num_encoder_self_attention_layers_per_block=1, num_encoder_cross_attention_heads=1,
              num_encoder_self_attention_heads=1, num_decoder_cross_attention_heads=1)
    with pytest.raises(ValueError, match="vocab_size"):
        LitMaskedLanguageModel(vocab_size=400, whole_word_masking=True, tokenizer_path=TOKENIZER, **kw)
    with pytest.raises(FileNotFoundError):
        LitMaskedLanguageModel(vocab_size=400, whole_word_masking=True, **kw)
    off = LitMaskedLanguageModel(vocab_size=V, mask_p=0.2, **kw)
    on = LitMaskedLanguageModel(vocab_size=V, whole_word_masking=True, word_clump=1.5, **kw)
    assert off.model.masking.mask_p == 0.2 and not off.model.masking.whole_word and off.model.masking.word_clump == 1.0
    assert on.model.masking.word_clump == 1.5
    assert list(on.state_dict()) == list(off.state_dict())
    # hyper-parameters of a checkpoint from before the options: the defaults
    old = {k: v for k, v in off.hparams.items()
           if k not in ("whole_word_masking", "mask_p", "word_clump", "tokenizer_path")}
    m = LitMaskedLanguageModel(**old)
    assert not m.model.masking.whole_word and m.model.masking.mask_p == 0.15


def test_mlm_cli_fit_with_whole_word_masking(tmp_path):
    """``scripts/mlm.py fit --model.whole_word_masking=true`` on synthetic text tokenized with the
    shipped vocabulary; the checkpoint keeps the flag and has the state-dict keys of a plain model."""
    from perceiver_io_amd.cli.tasks import main as cli_main
    from perceiver_io_amd.tasks import LitMaskedLanguageModel
    from perceiver_io_amd.train.checkpoint import load_checkpoint

    flags = ["fit", "--data=IMDBDataModule", "--data.synthetic=true", "--data.synthetic_size=32",
             "--data.vocab_size=10003", f"--data.tokenizer_path={TOKENIZER}", "--data.max_seq_len=48",
             "--data.batch_size=8", "--data.num_workers=0", "--data.data_dir=" + str(tmp_path / "cache"),
             "--model.num_latents=8", "--model.num_latent_channels=16", "--model.num_encoder_layers=1",
             "--model.num_encoder_self_attention_layers_per_block=1", "--model.num_encoder_cross_attention_heads=1",
             "--model.num_encoder_self_attention_heads=1", "--model.num_decoder_cross_attention_heads=1",
             "--model.whole_word_masking=true", "--model.mask_p=0.2", "--model.word_clump=2.5",
             f"--model.tokenizer_path={TOKENIZER}", "--model.masked_samples=null",
             "--optimizer.lr=0.003", "--trainer.max_epochs=1", "--trainer.max_steps=4",
             "--trainer.val_check_interval=2", "--trainer.limit_val_batches=1"]
    old = os.getcwd()
    os.chdir(tmp_path)
    try:
        cli = cli_main("mlm", flags)
    finally:
        os.chdir(old)
    assert cli.trainer.global_step == 4
    masking = cli.model.model.masking
    assert masking.whole_word and masking.mask_p == 0.2 and masking.word_clump == 2.5
    ck = [c for c in cli.trainer.callbacks if type(c).__name__ == "ModelCheckpoint"][0]
    assert os.path.exists(ck.best_model_path)
    hp = load_checkpoint(ck.best_model_path)["hyper_parameters"]
    assert hp["whole_word_masking"] is True and hp["mask_p"] == 0.2 and hp["word_clump"] == 2.5
    back = LitMaskedLanguageModel.load_from_checkpoint(ck.best_model_path)
    assert back.model.masking.whole_word and torch.equal(back.model.masking.word_table, masking.word_table)
    plain = LitMaskedLanguageModel(**{**hp, "whole_word_masking": False})
    assert list(back.state_dict()) == list(plain.state_dict())
    assert all(torch.equal(v, cli.model.state_dict()[k].cpu()) for k, v in back.state_dict().items())
