"""The contact head's CLI route without a GPU: the chunk plan, the config key, the ABI's declarations and the refusals that need no
device (every one of them comes before the first launch)."""
import ctypes
import os
import re

from rnamsm import _lib, contacts
from rnamsm.config import Config, parse_overrides

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rnamsm_contact_head_atp", "rnamsm_contact_head_packed_workspace_bytes", "rnamsm_contact_head_packed")


def test_plan_contact_chunks_respects_both_caps_and_keeps_order():
    Ls = [35, 64, 1, 128, 256, 7, 1023, 2, 2, 2]
    for max_pixels, max_batch in ((contacts.CONTACT_CHUNK_PIXELS, _lib.CONTACT_MAX_BATCH), (5000, 1024), (10 ** 9, 3), (1, 1024), (70000, 2)):
        chunks = contacts.plan_contact_chunks(Ls, max_pixels, max_batch)
        assert [i for c in chunks for i in c] == list(range(len(Ls)))                       # every index once, in list order
        for c in chunks:
            assert 1 <= len(c) <= max_batch
            assert sum(Ls[i] ** 2 for i in c) <= max_pixels or len(c) == 1                  # an oversized alignment is alone
        for a, b in zip(chunks, chunks[1:]):                                                # greedy: no two neighbours could be one
            assert len(a) + 1 > max_batch or sum(Ls[i] ** 2 for i in a) + Ls[b[0]] ** 2 > max_pixels
    assert contacts.plan_contact_chunks([]) == []
    assert contacts.plan_contact_chunks([5] * 1500) == [list(range(1024)), list(range(1024, 1500))]
    assert contacts.CONTACT_CHUNK_PIXELS == 1024 * 1024                                     # the SS head's order


def test_the_config_key_parses_and_defaults_to_off():
    assert Config().data.contacts is False
    assert parse_overrides(["data.contacts=true"]).data.contacts is True
    assert parse_overrides(["data.contacts=false"]).data.contacts is False
    assert parse_overrides([]).data.contacts is False


def test_the_new_symbols_are_declared_in_the_header_and_bound_with_matching_arity():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rnamsm.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\b(rnamsm_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S))
    for name in NEW + ("rnamsm_contact_head", "rnamsm_contact_head_workspace_bytes"):
        assert name in protos and name in _lib.EXPORTED_SYMBOLS, name
        assert len(protos[name].split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert "RNAMSM_CONTACT_MAX_L 1023" in header and f"RNAMSM_CONTACT_MAX_BATCH {_lib.CONTACT_MAX_BATCH}" in header
    assert _lib.CONTACT_MAX_L == 1023
    # rnamsm_contact_item as the header lays it out: pointer, int64, int32 (+ padding), pointer
    item = re.search(r"typedef struct \{([^}]*)\} rnamsm_contact_item;", header).group(1)
    assert [f.split()[-1] for f in item.split(";") if f.strip()] == [n for n, _ in _lib.ContactItem._fields_]
    assert ctypes.sizeof(_lib.ContactItem) == 32 and _lib.ContactItem.contacts.offset == 24


def test_sizes_and_refusals_that_need_no_device():
    lib = _lib.load()
    size = lib.rnamsm_contact_head_packed_workspace_bytes
    Ls = (ctypes.c_int * 3)(5, 300, 1)
    assert size(3, Ls, 120) == 256 + 4 * sum(120 * L + 120 for L in (5, 300, 1))
    assert size(3, Ls, 120) - 256 == sum(lib.rnamsm_contact_head_workspace_bytes(L + 1, 120) for L in (5, 300, 1))
    assert size(0, Ls, 120) == 0 and size(1025, Ls, 120) == 0 and size(3, None, 120) == 0 and size(3, Ls, 0) == 0
    assert size(3, (ctypes.c_int * 3)(5, 1024, 1), 120) == 0 and size(3, (ctypes.c_int * 3)(5, 0, 1), 120) == 0
    fake = ctypes.c_void_p(0x1000)                      # never dereferenced: every call below is refused on the host
    items = (_lib.ContactItem * 2)(_lib.ContactItem(0x1000, 25, 5, 0x2000), _lib.ContactItem(0x3000, 8, 3, 0x4000))

    def refused(rc, *words):
        assert rc == -1, rc
        msg = lib.rnamsm_last_error().decode()
        assert all(w in msg for w in words), msg

    refused(lib.rnamsm_contact_head_packed(items, 2, 120, fake, fake, fake, 1 << 30, None), "contact_head_packed", "member 1", "plane stride")
    refused(lib.rnamsm_contact_head_packed(items, 1, 120, fake, fake, fake, 16, None), "contact_head_packed", "workspace too small")
    refused(lib.rnamsm_contact_head_packed(items, 1, 120, fake, fake, ctypes.c_void_p(0x1004), 1 << 30, None), "16-byte")
    refused(lib.rnamsm_contact_head_atp(fake, 24, 5, 120, fake, fake, fake, fake, 1 << 30, None), "contact_head_atp", "plane stride")
    refused(lib.rnamsm_contact_head_atp(fake, 25, 5, 120, fake, fake, fake, fake, 4 * (120 * 5 + 120) - 1, None), "workspace too small")
