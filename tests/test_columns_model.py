"""CPU: the columnar decode's host side -- ysb_columns_layout_of against the reference
constructor's arithmetic (AdvertisingTopologyNative.java:291-302), the ctypes mirror of the
two structs, the null-argument errors -- and the CPU model's own checks: the mutation corpus
the GPU tests decode is tagged, the tags agree with oracle/dostats.py, and it is balanced."""
import ctypes as C

import pytest

import columns_model as cm
import golden_data as gd
from oracle import dostats
from ysb_amd import _lib, columns_layout


def gen_lines(n=None):
    raw, _ = gd.events("gen_s7")
    lines, _ = dostats.split_lines(raw)
    return lines[:n] if n else lines


def test_layout_worked_case_5000():
    lay = columns_layout(5000)   # the fork's window.size
    assert lay["start"][:7] == [0, 180224, 360448, 540672, 561152, 581632, 622592]
    assert lay["image_bytes"] == 663552 == lay["start"][7]
    assert lay["start"][8] == 663552 + 4096
    assert lay["width"] == [36, 36, 36, 4, 4, 8, 8] and lay["rows"] == 5000


@pytest.mark.parametrize("rows", [1, 64, 65, 113, 114, 4096, 5000, 32768, 32769, (1 << 31) - 1])
def test_layout_matches_model(rows):
    lay, m = columns_layout(rows), cm.layout(rows)
    assert lay["start"] == m["start"] and lay["image_bytes"] == m["image_bytes"]
    assert all(s % 4096 == 0 for s in lay["start"])
    for j in range(7):
        assert lay["start"][j + 1] - lay["start"][j] >= cm.WIDTH[j] * rows
    assert lay["start"][8] - lay["start"][7] >= (rows + 63) // 64 * 8


def test_layout_small_rows():
    for rows in (1, 64, 65):
        lay = columns_layout(rows)
        assert lay["start"] == [4096 * j for j in range(9)]   # every buffer fits one page


def test_layout_argument_errors():
    L = _lib.lib()
    lay = _lib.YsbColumnsLayout()
    assert L.ysb_columns_layout_of(0, C.byref(lay)) == -1
    assert L.ysb_columns_layout_of(1 << 31, C.byref(lay)) == -1
    assert L.ysb_columns_layout_of((1 << 31) - 1, C.byref(lay)) == 0
    assert L.ysb_columns_layout_of(5000, None) == -1


def test_structs_and_signatures():
    assert C.sizeof(_lib.YsbColumnsLayout) == 8 + 72 + 28 + 4 + 8
    assert _lib.YsbColumnsLayout.start.offset == 8 and _lib.YsbColumnsLayout.width.offset == 80
    assert _lib.YsbColumnsLayout.image_bytes.offset == 112
    assert C.sizeof(_lib.YsbDecodeInfo) == 32 and _lib.YsbDecodeInfo.kernel_ms.offset == 24
    assert _lib.YSB_COL_JAVA_ORDER == 1
    for f in ("ysb_columns_layout_of", "ysb_decode_columns_device"):
        assert f in _lib.SIGNATURES and hasattr(_lib.lib(), f)
    assert len(_lib.SIGNATURES["ysb_decode_columns_device"][1]) == 10


def test_decode_null_context_is_an_argument_error():
    info = _lib.YsbDecodeInfo()
    assert _lib.lib().ysb_decode_columns_device(None, None, 0, None, 0, None, 64, 10, 0, C.byref(info)) == -1


def test_model_rows():
    lines = gen_lines(3)
    img, valid, info = cm.build(lines, batch_rows=5)
    st = cm.layout(5)["start"]
    assert valid.all() and info == {"rows": 3, "valid": 3}
    d = [cm._fields(ln) for ln in lines]
    assert bytes(img[st[0]:st[0] + 36]) == d[0]["user_id"].encode()
    assert bytes(img[st[2] + 36:st[2] + 72]) == d[1]["ad_id"].encode()
    assert bytes(img[st[3]:st[3] + 4]) == b"bann" and bytes(img[st[4] + 4:st[4] + 8]) == b"clic"   # cut at the width
    assert int.from_bytes(bytes(img[st[5] + 16:st[5] + 24]), "little") == int(d[2]["event_time"])
    assert int.from_bytes(bytes(img[st[6]:st[6] + 8]), "little") == 10
    assert img[st[7]] == 0b111 and not img[st[7] + 1:].any()
    assert not img[st[0] + 3 * 36:st[1]].any()
    big, _, _ = cm.build(lines, batch_rows=5, java_order=True, stamp=-2)
    assert int.from_bytes(bytes(big[st[5] + 16:st[5] + 24]), "big") == int(d[2]["event_time"])
    assert int.from_bytes(bytes(big[st[6]:st[6] + 8]), "big", signed=True) == -2
    same = [slice(0, st[5]), slice(st[7], st[8])]
    assert all((img[s] == big[s]).all() for s in same)
    can, _, _ = cm.build(lines, batch_rows=5, canary=0xA5)
    assert (can[st[0] + 3 * 36:st[1]] == 0xA5).all() and (can[st[7] + 8:] == 0xA5).all()
    assert (can[st[7]:st[7] + 8] == img[st[7]:st[7] + 8]).all()


def test_mutation_corpus_tags_agree_with_the_oracle():
    corpus = cm.mutation_corpus(gen_lines())
    assert len(cm.CLASSES) == 18
    assert sum(ok for _, ok, _ in cm.CLASSES) == 12
    for ln, name, ok in corpus:
        assert (cm.decode_line(ln) is not None) == ok, (name, ln)
        want_ip = ok and name not in cm.NEEDS_IP
        assert (cm.decode_line(ln, require_ip=True) is not None) == want_ip, (name, ln)
    n_valid = sum(ok for _, _, ok in corpus)
    assert 0.30 * len(corpus) <= n_valid <= 0.75 * len(corpus)


def test_mutation_corpus_keeps_the_values():
    lines = gen_lines(36)
    for (ln, name, ok), src in zip(cm.mutation_corpus(lines), lines):
        if not ok:
            continue
        d, (vals, t) = cm._fields(src), cm.decode_line(ln)
        assert vals[1] == d["page_id"].encode() and vals[2] == d["ad_id"].encode(), name
        assert t == int(d["event_time"]), name
        if name == "two_byte_user_id_36":
            assert vals[0] == ("é" * 17 + "ab").encode() and len(vals[0]) == 36
        elif name == "u_escape_user_id":
            assert vals[0] == d["user_id"].encode() and b"\\u00" in ln
        if name == "escaped_slash_ad_type":
            assert vals[3] == (d["ad_type"][:2] + "/" + d["ad_type"][2:])[:4].encode()


def test_edge_fixtures_are_usable():
    raw, _ = gd.events("edge")
    lines, _ = dostats.split_lines(raw)
    assert len(lines) == 54 and sum(cm.decode_line(ln) is not None for ln in lines) == 28
    raw, _ = gd.events("gen_s7", ".tbl")
    lines, _ = dostats.split_lines(raw)
    assert all(cm.decode_line(ln, fmt="tbl") is not None for ln in lines)
