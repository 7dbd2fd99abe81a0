"""Host logic of long-form synthesis (text2speech_amd/longform.py) and the argument checks of audio.join_batches and
longform.synthesize_long that need no device."""
import types

import pytest
import torch

from text2speech_amd import _lib, audio, longform as L
from text2speech_amd.text import text_to_sequence

T2SError = _lib.T2SError


def _rejoins(text, chunks):
    assert " ".join(chunks) == " ".join(text.split())
    assert all(c and c == c.strip() for c in chunks)


# ------------------------------------------------------------------------------------------------------------------ split_text
def test_split_sentences_korean_ascii_and_full_width():
    text = "안녕하세요.  오늘은 날씨가 좋습니다!\n정말요？ 네。 Hello there. How are you?  끝"
    chunks = L.split_text(text)
    assert chunks == ["안녕하세요.", "오늘은 날씨가 좋습니다!", "정말요？", "네。", "Hello there.", "How are you?", "끝"]
    _rejoins(text, chunks)


def test_a_mark_cuts_only_where_whitespace_or_the_end_follows():
    assert L.split_text("a.b c. d") == ["a.b c.", "d"]
    assert L.split_text("3.14 is pi. Yes.") == ["3.14 is pi.", "Yes."]
    assert L.split_text("끝.") == ["끝."]


def test_empty_pieces_are_dropped():
    assert L.split_text("") == [] and L.split_text("  \n\t ") == []
    assert L.split_text(" 네.   ") == ["네."]


def test_long_sentence_is_cut_at_commas_then_at_whitespace():
    s = "하나, 둘 셋 넷 다섯; 여섯 일곱: 여덟 아홉 열."
    assert L.n_symbols(s) == len(text_to_sequence(s)) == 56
    assert L.split_text(s, 56) == [s]
    # at the clause marks only, neighbours put together again while they fit; the mark stays on the left
    assert L.split_text(s, 40) == ["하나, 둘 셋 넷 다섯; 여섯 일곱:", "여덟 아홉 열."]
    assert L.split_text(s, 20) == ["하나,", "둘 셋 넷 다섯;", "여섯 일곱:", "여덟 아홉 열."]
    # "둘 셋 넷 다섯;" is 19 symbols: at 12 it is cut at whitespace
    assert L.split_text(s, 12) == ["하나,", "둘 셋 넷", "다섯;", "여섯", "일곱:", "여덟 아홉", "열."]
    for m in (56, 40, 20, 12, 8):
        chunks = L.split_text(s, m)
        _rejoins(s, chunks)
        assert max(L.n_symbols(c) for c in chunks) <= m


def test_full_width_clause_marks():
    s = "하나， 둘 셋； 넷 다섯、 여섯."
    assert L.split_text(s, 10) == ["하나，", "둘 셋；", "넷 다섯、", "여섯."]


def test_a_word_too_long_to_cut_is_refused():
    with pytest.raises(ValueError, match="without whitespace"):
        L.split_text("하나, 가나다라마바사아자차카타파하 둘.", 12)
    with pytest.raises(ValueError):
        L.split_text("abc", 1)
    with pytest.raises(ValueError):
        L.split_text(["abc"])


@pytest.mark.parametrize("m", [14, 16, 33, 64])          # (the longest word is 14 symbols)
def test_rejoin_property(m):
    text = ("  서울은 대한민국의 수도이다. 인구는 약 천만 명이며,  한강이 도시를 가로지른다; 날씨는\n사계절이 뚜렷하다! "
            "What about winter? It is cold: very cold, and dry.  끝")
    chunks = L.split_text(text, m)
    _rejoins(text, chunks)
    assert max(L.n_symbols(c) for c in chunks) <= m


# ----------------------------------------------------------------------------------------------------------------- chunk_seeds
# s_i = mix((i + 1) GOLD + seed) >> 1 with include/t2s_hip.h's mix and GOLD, computed once with Python ints
SEEDS_OF = {
    0: [8147104208329303767, 3980143261097177850, 243808509735772839, 8954805688390271222],
    20240611: [223763391278328891, 8877849913091432248, 1979449017150588136, 878377662046355150],
    2 ** 63 - 1: [1527823816519176019, 8720658416722345123, 8505832573251952840, 1157452369933151741],
}


@pytest.mark.parametrize("seed", sorted(SEEDS_OF))
def test_chunk_seeds_values(seed):
    got = L.chunk_seeds(seed, 4)
    assert got == SEEDS_OF[seed] and all(type(s) is int for s in got)
    assert L.chunk_seeds(seed, 2) == SEEDS_OF[seed][:2] and L.chunk_seeds(seed, 0) == []


def test_chunk_seeds_range_and_separation():
    for seed in (0, 1, 977, 2 ** 63 - 1):
        a, b = L.chunk_seeds(seed, 64), L.chunk_seeds(min(seed + 1, 2 ** 63 - 1) if seed < 2 ** 63 - 1 else seed - 1, 64)
        assert all(0 <= s < 2 ** 63 for s in a)
        assert len(set(a)) == 64 and not set(a) & set(b)
    for bad in (-1, 2 ** 63, 1.5, None):
        with pytest.raises(ValueError):
            L.chunk_seeds(bad, 3)


# ------------------------------------------------------------------------------------------------------- milliseconds -> samples
def test_ms_to_samples():
    assert L.ms_to_samples(250, 44800) == 11200
    assert L.ms_to_samples(5, 44800) == 224
    assert L.ms_to_samples(0, 44800) == 0
    assert L.ms_to_samples(0.01, 44800) == 0 and L.ms_to_samples(0.02, 44800) == 1        # 0.448 and 0.896 samples
    assert L.ms_to_samples(12.5, 22050) == round(12.5 * 22050 / 1000) == 276
    assert type(L.ms_to_samples(3.3, 48000)) is int
    for bad in (-1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            L.ms_to_samples(bad, 44800)


def test_plan_groups_and_order():
    n_ids = [5, 9, 3, 9, 7]
    groups, order = L._plan(n_ids, 2, True)
    assert groups == [[1, 3], [4, 0], [2]]                      # decreasing id count, equal counts in the text's order
    assert order == [3, 0, 4, 1, 2]                             # chunk p is row order[p]
    rows = [c for g in groups for c in g]
    assert [rows[r] for r in order] == [0, 1, 2, 3, 4]
    groups, order = L._plan(n_ids, 8, False)
    assert groups == [[0, 1, 2, 3, 4]] and order == [0, 1, 2, 3, 4]


# --------------------------------------------------------------------------------------------------- join_batches: no device
def test_join_batches_argument_checks_without_a_device():
    x = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="HBM"):
        audio.join_batches([(x, [8, 8])])                       # a CPU tensor
    with pytest.raises(RuntimeError, match="HBM"):
        audio.join_batch(x, [8, 8])
    with pytest.raises(T2SError):
        audio.join_batches([])
    with pytest.raises(T2SError):
        audio.join_batches([(x,)])
    with pytest.raises(T2SError):
        audio.join_batches(x)
    for kw in (dict(fade=-1), dict(fade=65537), dict(fade=1.5), dict(fade=True)):
        with pytest.raises(ValueError):
            audio.join_batches([(x, [8, 8])], **kw)


class _FakeCuda:
    """what _join_rows reads of a tensor, reporting itself as one in HBM: the checks behind the device check, without a device"""

    def __init__(self, t, device="cuda:0"):
        self._t, self.is_cuda, self.device = t, True, torch.device(device)
        self.dtype, self.shape = t.dtype, t.shape

    def dim(self):
        return self._t.dim()

    def size(self, i):
        return self._t.size(i)

    def numel(self):
        return self._t.numel()

    def detach(self):
        return self

    def reshape(self, *a):
        return _FakeCuda(self._t.reshape(*a), self.device)


def test_join_batches_argument_checks_behind_the_device_check(monkeypatch):
    monkeypatch.setattr(audio, "_need_cuda", lambda t, what: None)
    monkeypatch.setattr(audio, "_to_device", lambda *a: (_ for _ in ()).throw(AssertionError("reached the device")))
    f32 = _FakeCuda(torch.zeros(2, 8))
    ok = [(f32, [8, 3])]
    with pytest.raises(T2SError, match="float32 or float16"):
        audio.join_batches([(_FakeCuda(torch.zeros(2, 8, dtype=torch.float64)), [8, 8])])
    with pytest.raises(T2SError, match="float32 or float16"):
        audio.join_batches([(_FakeCuda(torch.zeros(2, 8, dtype=torch.int16)), [8, 8])])
    with pytest.raises(T2SError, match=r"\[B, N\]"):
        audio.join_batches([(_FakeCuda(torch.zeros(8)), [8])])
    with pytest.raises(T2SError, match=r"\[B, N\]"):
        audio.join_batches([(_FakeCuda(torch.zeros(2, 2, 8)), [8, 8])])
    with pytest.raises(T2SError, match="lengths"):
        audio.join_batches([(f32, [8, 8, 8])])
    with pytest.raises(T2SError, match="integers"):
        audio.join_batches([(f32, [8.0, 8.0])])
    with pytest.raises(T2SError, match="batch 1 is on"):
        audio.join_batches([(f32, [8, 8]), (_FakeCuda(torch.zeros(1, 4), "cuda:1"), [4])])
    for order in ([0, 0], [0], [0, 1, 2], [1, 2], [-1, 0], [0.0, 1.0]):
        with pytest.raises(ValueError, match="order"):
            audio.join_batches(ok, order=order)
    for pauses in ([], [1, 2], [-1], [0.5]):
        with pytest.raises(ValueError, match="pause"):
            audio.join_batches(ok, pauses=pauses)
    with pytest.raises(ValueError, match="pause"):
        audio.join_batches(ok, pause=-3)
    with pytest.raises(T2SError, match="the most is"):
        audio.join_batches(ok, pause=2 ** 31)
    # a valid call gets as far as the first copy to the device
    with pytest.raises(AssertionError, match="reached the device"):
        audio.join_batches(ok, order=[1, 0], pauses=[4], fade=3, fade_ends=True)


# ------------------------------------------------------------------------------------------------ synthesize_long: no device
def _models(training=False):
    return types.SimpleNamespace(training=training), types.SimpleNamespace(training=False)


def test_synthesize_long_refusals_without_a_device():
    t, w = _models()
    with pytest.raises(T2SError, match="seed"):
        L.synthesize_long(t, w, "안녕.")                        # no seed
    with pytest.raises(T2SError, match="seed"):
        L.synthesize_long(t, w, "안녕.", seed=1, seeds=[1])     # both
    with pytest.raises(T2SError, match="exactly one"):
        L.synthesize_long(t, w, "안녕.", chunks=["안녕."], seed=1)
    with pytest.raises(T2SError, match="exactly one"):
        L.synthesize_long(t, w, seed=1)
    with pytest.raises(T2SError, match="nothing to say"):
        L.synthesize_long(t, w, "  \n ", seed=1)
    with pytest.raises(T2SError, match="nothing to say"):
        L.synthesize_long(t, w, chunks=[], seed=1)
    with pytest.raises(T2SError, match="not one string"):
        L.synthesize_long(t, w, chunks="안녕.", seed=1)
    with pytest.raises(T2SError, match="strings"):
        L.synthesize_long(t, w, chunks=[[3, 4, 1]], seed=1)
    with pytest.raises(T2SError, match="eval mode"):
        L.synthesize_long(*_models(training=True), "안녕.", seed=1)
    with pytest.raises(ValueError, match="seeds holds 1"):
        L.synthesize_long(t, w, "안녕. 네.", seeds=[1])
    with pytest.raises(ValueError):
        L.synthesize_long(t, w, "안녕. 네.", seeds=[1, -2])
    with pytest.raises(ValueError):
        L.synthesize_long(t, w, "안녕.", seed=2 ** 63)
    with pytest.raises(ValueError, match="batch_size"):
        L.synthesize_long(t, w, "안녕.", seed=1, batch_size=0)
    with pytest.raises(ValueError, match="pauses_ms holds 2"):
        L.synthesize_long(t, w, "안녕. 네.", seed=1, pauses_ms=[10, 10])
    for kw in (dict(pause_ms=-1), dict(fade_ms=-0.5), dict(pauses_ms=[float("nan")]), dict(sampling_rate=0)):
        with pytest.raises(ValueError):
            L.synthesize_long(t, w, "안녕. 네.", seed=1, **kw)
    with pytest.raises(ValueError, match="without whitespace"):
        L.synthesize_long(t, w, "가나다라마바사아자차카타파하", seed=1, max_symbols=8)


def test_check_long_args_results():
    t, w = _models()
    chunks, ids, seeds, gaps, fade = L._check_long_args(t, w, "안녕. 네? 끝", None, 7, None, 8, 64, 250, None, 5, 44800)
    assert chunks == ["안녕.", "네?", "끝"] and seeds == L.chunk_seeds(7, 3)
    assert [i.tolist() for i in ids] == [text_to_sequence(c).tolist() for c in chunks]
    assert gaps == [11200, 11200] and fade == 224
    chunks, ids, seeds, gaps, fade = L._check_long_args(t, w, None, ["네. 네.", "끝"], None, [5, 6], 1, 64, 250, [12.5], 0, 22050)
    assert chunks == ["네. 네.", "끝"] and seeds == [5, 6] and gaps == [276] and fade == 0       # chunks are not split again
