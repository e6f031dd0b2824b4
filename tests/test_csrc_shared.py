"""The helpers the three libraries share (snappy.jl_amd/csrc/common/) exist once: a second copy of
the byte mover, the block scan, the device buffer or the scratch carver under csrc/ fails here, and
so does a scratch size kept as a constant beside its carve.  Reads sources only."""
import functools
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "snappy.jl_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _sources():
    out = {}
    for d, _, files in os.walk(CSRC):
        if os.path.basename(d).startswith("build"):
            continue
        for f in files:
            if f.endswith((".hip", ".h", ".cpp", ".mk")) or f == "Makefile":
                p = os.path.join(d, f)
                text = open(p).read()
                text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
                out[os.path.relpath(p, CSRC)] = re.sub(r"//[^\n]*", "", text)
    return out


def _definitions(pattern):
    return sorted(f for f, text in _sources().items() for _ in re.finditer(pattern, text))


def test_shared_directory_is_read():
    names = set(_sources())
    assert {"sm_api.hip", "framing/smf_kernels.hip", "framing/smf_range.hip", "multi/smm_kernels.hip",
            "common/companion.mk"} <= names


def test_device_helpers_have_one_definition():
    for name in ("copy_bytes", "block_scan", "sat32"):
        # a function definition: a return type before the name, a body behind the parameters
        found = _definitions(r"\b[\w:]+[\s\*&]+%s\s*\([^;{}]*\)\s*\{" % name)
        assert len(found) == 1 and found[0].startswith("common/"), (name, found)


def test_host_helpers_have_one_definition():
    for pattern in (r"\bstruct\s+DevBuf\b\s*\{", r"\bstruct\s+DeviceGuard\b\s*\{", r"\bstruct\s+\w*Carve\w*\s*\{",
                    r"\b[\w:]+\s+valid_mode\s*\([^;{}]*\)\s*\{", r"#\s*define\s+\w*_CHECK\s*\(", r"#\s*define\s+\w*_PASS\s*\("):
        found = _definitions(pattern)
        assert len(found) == 1 and found[0].startswith("common/"), (pattern, found)
    assert _definitions(r"\bstruct\s+\w*Carve\w*\s*\{") == _definitions(r"\bstruct\s+Carve\s*\{")


def test_no_scratch_size_beside_its_carve():
    for name in ("RangeCarve", "kCompressMeta", "kDecodeMeta", "kIndexMeta"):
        found = _definitions(r"\b%s\b" % name)
        assert not found, (name, found)
    found = _definitions(r"\bmeta_bytes\b")
    assert not found, found


def test_host_rules_have_one_definition_without_hip():
    """What sm_api.hip decides from untrusted bytes lives in sm_host_rules.h, which (with
    sm_format.h) the host compiler alone builds for the sanitizer driver."""
    for name in ("literal_only", "host_walk", "make_shards", "small_chunk", "check_compressed_lengths"):
        found = _definitions(r"\b[\w:<>]+[\s\*&]+%s\s*\([^;{}]*\)\s*\{" % name)
        assert found == ["sm_host_rules.h"], (name, found)
    for f in ("sm_host_rules.h", "sm_format.h"):
        assert not re.search(r"#\s*include\s*[<\"]hip/", _sources()[f]), f


def test_format_rules_have_one_definition():
    """The rules every walker applies to untrusted bytes -- one tag, the reference's three checks,
    the varint header -- are written once: decode_tag and check_tag in sm_format.h, varint_len and
    parse_varint32 in common/smc_layout.h, and the trailer mask in sm_format.h alone."""
    for name, where in (("decode_tag", "sm_format.h"), ("check_tag", "sm_format.h"), ("window_out_bytes", "sm_format.h"),
                        ("varint_len", "common/smc_layout.h"), ("parse_varint32", "common/smc_layout.h")):
        found = _definitions(r"\b[\w:<>]+[\s\*&]+%s\s*\([^;{}]*\)\s*\{" % name)
        assert found == [where], (name, found)
    for name in ("parse_varint", "parse_header32"):  # the companions' former copies
        assert not _definitions(r"\b[\w:<>]+[\s\*&]+%s\s*\(" % name), name
    mask = [f for f, text in _sources().items() if re.search(r"1u\s*<<\s*\(\s*8\s*\*\s*\w*\.?taglen\s*\)", text)]
    assert mask == ["sm_format.h"], mask
    # a varint parse is a loop over (b & 0x7f) << (7 * i): one file (beside the host checkers, whose
    # expected values never come from the code under test)
    loops = [f for f, text in _sources().items()
             if re.search(r"0x7f\s*\)\s*<<\s*\(\s*7\s*\*", text) and not f.endswith("_check.cpp")]
    assert loops == ["common/smc_layout.h"], loops


def test_decoder_files_are_in_the_version_hash():
    """sm_dec_walk.h and sm_dec_stream.hip enter the Makefile's HDRS and SRCS, so the version string
    changes with them and every object is rebuilt when the shared walk changes."""
    mk = _sources()["Makefile"]
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1).split()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "sm_dec_walk.h" in hdrs and {"sm_decompress.hip", "sm_dec_stream.hip"} <= set(srcs)
    hips = {f for f in _sources() if f.endswith(".hip") and "/" not in f}
    assert hips == set(srcs), (hips, srcs)


def test_framing_rules_have_one_definition():
    """The framing library's decode entry points share one slot stage: the two verdict rules, the
    scan of the groups' slot counts, the chunk walk, the index check and the one-wave fetch are
    written once under csrc/framing/, and the copies they replaced are gone."""
    framing = {f: text for f, text in _sources().items() if f.startswith("framing/")}
    for name, where in (("slot_verdict", "framing/smf_slots.h"), ("group_verdict", "framing/smf_slots.h"),
                        ("scan_counts", "framing/smf_device.h"), ("walk_stream", "framing/smf_format.h"),
                        ("valid_chunks", "framing/smf_format.h")):
        found = sorted(f for f, text in framing.items()
                       for _ in re.finditer(r"\b[\w:<>]+[\s\*&]+%s\s*\([^;{}]*\)\s*\{" % name, text))
        assert found == [where], (name, found)
    # ... and scan_counts is a forwarder: the scan itself is defined once in all of csrc/, in common/
    found = _definitions(r"\b[\w:<>]+[\s\*&]+count_scan\s*\([^;{}]*\)\s*\{")
    assert found == ["common/smc_device.h"], found
    assert len(re.findall(r"\btile_scan\b", framing["framing/smf_device.h"])) == 0
    fetch = sorted(f for f, text in framing.items() for _ in re.finditer(r"\bstruct\s+WaveFetch\b\s*\{", text))
    assert fetch == ["framing/smf_device.h"], fetch
    for f in ("framing/smf_slots.h", "framing/smf_format.h"):  # the sanitizer driver compiles them for the host
        assert not re.search(r"#\s*include\s*[<\"]hip/", framing[f]), f
    # walk_step is called by walk_stream, the one loop around it -- and by k_frame_index, which keeps
    # that loop and the fetch written out because the shared form measured slower there
    calls = sorted(f for f, text in framing.items() if not f.endswith("_check.cpp")
                   for _ in re.finditer(r"(?<![\w:])(?:smf::)?walk_step\s*\((?!Walk&)", text))
    assert calls == ["framing/smf_format.h", "framing/smf_kernels.hip"], calls
    shuffles = sorted(f for f, text in framing.items() for _ in re.finditer(r"__shfl\s*\(", text))
    assert shuffles == ["framing/smf_device.h", "framing/smf_kernels.hip"], shuffles
    for name in ("RangeHeader", "StreamsHeader", "DecodeMeta", "k_range_scan", "k_range_verify", "k_streams_verify",
                 "k_frame_verify", "k_range_copy", "k_frame_copy", "k_range_result", "k_streams_result"):
        found = [f for f, text in framing.items() if re.search(r"\b%s\b" % name, text)]
        assert not found, (name, found)


def test_framing_headers_are_in_the_version_hash():
    mk = _sources()["framing/Makefile"]
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1).split()
    here = {f.split("/", 1)[1] for f in _sources() if f.startswith("framing/") and f.endswith(".h")}
    assert here and here <= set(hdrs), (here, hdrs)


def test_emit_rules_have_one_definition():
    """What a compressor writes for one token is written once, beside its decode twin: the varint
    byte in common/smc_layout.h; the literal tag (with the reference's Q3 rule as a named choice),
    the copy piece, emit_copy!'s split, the closed form of its size, a block as one literal and the
    verdict over a block's parts in sm_format.h.  The kernels call them; none restates one."""
    src = _sources()
    for name, where in (("varint_byte", "common/smc_layout.h"), ("literal_tag", "sm_format.h"),
                        ("literal_tag1", "sm_format.h"), ("literal_tag_bytes", "sm_format.h"), ("copy_piece", "sm_format.h"),
                        ("copy_piece_len", "sm_format.h"), ("copy_tag_bytes", "sm_format.h"),
                        ("block_literal_bytes", "sm_format.h"), ("block_literal_head_byte", "sm_format.h"),
                        ("parts_verdict", "sm_format.h")):
        found = _definitions(r"\b[\w:<>]+[\s\*&]+%s\s*\([^;{}]*\)\s*\{" % name)
        assert found == [where], (name, found)
    assert not re.search(r"#\s*include\s*[<\"]hip/", src["sm_format.h"])
    product = {f: text for f, text in src.items() if not f.endswith("_check.cpp")}
    forms = {
        "varint byte": r"&\s*0x7f\s*\)\s*\|\s*\([^;]*\?\s*0x80",
        "literal tag": r"\(\s*5[89]\s*\+\s*\w+\s*\)\s*<<\s*2|\b6[0-3]u?\s*<<\s*2",
        "copy-1 tag": r"&\s*0xe0",
    }
    where = {"varint byte": "common/smc_layout.h", "literal tag": "sm_format.h", "copy-1 tag": "sm_format.h"}
    for what, pattern in forms.items():
        found = sorted(f for f, text in product.items() if re.search(pattern, text))
        assert found == [where[what]], (what, found)
    # the one-byte literal tag's threshold is the named rule, not a `< 60` against a `<= 60` elsewhere
    assert re.search(r"enum\s+LiteralRule\b[^;]*kLiteralStd[^;]*kLiteralQ3", src["sm_format.h"])
    q3 = sorted(f for f, text in product.items() if "kLiteralQ3" in text)
    assert q3 == ["sm_compress.hip", "sm_format.h"], q3
    # the one-byte form alone (literal_tag1) is called where a run is known to be short: the fast parse's
    # runs inside one lane's 16 positions -- and by literal_tag itself
    short = sorted((f, len(re.findall(r"\bliteral_tag1\s*\(", text))) for f, text in product.items() if "literal_tag1" in text)
    assert short == [("sm_compress_sc.hip", 1), ("sm_format.h", 2)], short
    for f, text in product.items():  # no call passes the rule as a bare literal
        assert not re.search(r"\bliteral_tag\s*\([^()]*,\s*(?:0|1|true|false)\s*\)", text), f
    for name in ("cu_count", "kScreenTodoSc", "sc_lit_tag", "sc_copy_piece", "sc_copy_bytes", "put_copy_upto_64"):
        found = [f for f, text in src.items() if re.search(r"\b%s\b" % name, text)]
        assert not found, (name, found)
    for name, where_ in (("compress_grid", "sm_internal.h"), ("launch_screen", "sm_compress_fast.hip"),
                         ("sc_stage_block", "sm_compress_sc.hip"), ("sc_reset_handoff", "sm_compress_sc.hip")):
        found = _definitions(r"\b[\w:<>]+[\s\*&]+%s\s*\([^;{}]*\)\s*\{" % name)
        assert found == [where_], (name, found)
    sc = src["sm_compress_sc.hip"]
    assert len(re.findall(r"\bsc_stage_block\s*\(", sc)) == 3 and len(re.findall(r"\bsc_reset_handoff\s*\(", sc)) == 3
    assert len(re.findall(r"\blaunch_screen\s*\(", src["sm_compress_fast.hip"])) == 4  # the definition, three launchers
    for name in ("kScreenTodo", "kNotABlock"):
        found = _definitions(r"\bconstexpr\s+uint32_t\s+%s\s*=" % name)
        assert found == ["sm_internal.h"], (name, found)
    marks = sorted(f for f, text in product.items() if re.search(r"0xfff00000u|0xfffffffeu", text, re.I))
    assert marks == ["sm_format.h", "sm_internal.h"], marks
    # the batch parts gather decides by the one verdict.  The single-stream one keeps the rule in its
    # parallel form (a thread per part, a butterfly sum): on the single-buffer call's latency path the
    # rule as a loop per thread measured 2.5 to 3 us slower.  Exactly that one
    # restatement remains: the part-0 allowance and the butterfly occur once outside sm_format.h.
    assert len(re.findall(r"\bparts_verdict\s*\(", src["sm_gather.hip"])) == 1
    allowance = sorted((f, len(re.findall(r"\blit\s*\+\s*5u", text))) for f, text in product.items() if re.search(r"\blit\s*\+\s*5u", text))
    assert allowance == [("sm_format.h", 2), ("sm_gather.hip", 1)], allowance
    assert len(re.findall(r"__shfl_xor", src["sm_gather.hip"])) == 1
    for name in ("block_literal_bytes", "put_literal_head"):  # ... and its literal comes from the shared rules
        assert len(re.findall(r"\b%s\s*\(" % name, src["sm_gather.hip"])) >= 2, name
    assert re.search(r"\bk_gather_parts\s*\(", src["sm_gather.hip"]) and re.search(r"\bk_gather_parts_batch\s*\(", src["sm_gather.hip"])


def test_container_helpers_have_one_definition():
    """What the container libraries (framing, blocks, orc, parquet, avro, table) share exists once,
    under csrc/common/: the tiled scan and the count scan over it, the tiled copy, the slot rules
    (owner search, group rule, copy rows, round16), the host-buffer calls' staging and the two
    one-wave fetches that read lanes into scalar registers.  The framing library's __shfl fetch stays
    its own."""
    src = _sources()
    for name in ("tile_scan", "count_scan", "copy_tiled", "copy_grid", "copy_rows", "slot_owner", "plan_verdict", "round16",
                 "walker_index", "carve_stream_call", "upload_stream_call", "download_results", "download_output"):
        found = _definitions(r"\b[\w:<>]+[\s\*&]+%s\s*\([^;{}]*\)\s*\{" % name)
        assert len(found) == 1 and found[0].startswith("common/"), (name, found)
    for name in ("StreamStaging", "StreamCallArrays", "ArgUpload", "PlanHeader"):
        found = _definitions(r"\bstruct\s+%s\b\s*\{" % name)
        assert found == ["common/smc_staging.h"] or (name == "PlanHeader" and found == ["common/smc_slots.h"]), (name, found)
    for name in ("kNoSlot", "kCopyTile", "kCopyGroups", "kWalkWaves", "kWindow"):
        found = _definitions(r"\bconstexpr\s+uint32_t\s+%s\s*=" % name)
        # (the framing streams' walkers keep their own count of waves beside their own fetch; the multi
        # library's ranged decode has a mark of its own under that name)
        assert [f for f in found if f not in ("framing/smf_streams.hip", "multi/smm_range.h")] == ["common/smc_device.h" if name in ("kWalkWaves", "kWindow")
                                                                        else "common/smc_slots.h"], (name, found)
    # by their bodies, whatever a copy would be called: the binary search of a scan, the group rule,
    # the rounding, the tile loop, the staging's upload of a byte at the least
    forms = {
        "owner search": r"first\s*\[\s*mid\s*\]\s*<=\s*j",
        "group rule": r"fail\s*!=\s*\w+\s*\?\s*fail_status",
        "tile loop": r"blockIdx\.y\s*\*\s*kCopyTile",
        "count scan": r"total\s*=\s*over\s*\?\s*0u\s*:\s*\(uint32_t\)\s*sum",
        "staging ensure": r"io_out\s*\.\s*ensure\s*\(",
        "window fetch": r"pos\s*-\s*base\s*>=\s*kWindow",
    }
    where = {"owner search": "common/smc_slots.h", "group rule": "common/smc_slots.h", "tile loop": "common/smc_device.h",
             "count scan": "common/smc_device.h", "staging ensure": "common/smc_staging.h", "window fetch": "common/smc_device.h"}
    for what, pattern in forms.items():
        # (the multi library, which the containers sit on, keeps its own plan rules: smm_plan.h)
        found = sorted(f for f, text in src.items()
                       if re.search(pattern, text) and not f.endswith("_check.cpp") and not f.startswith("multi/"))
        # (the framing library's single-stream calls size their staging themselves: no batch, no arrays)
        found = [f for f in found if not (what == "staging ensure" and f == "framing/smf_api.hip")]
        # (the table library's k_tab_scan carries the index stage's `over` into its own: another rule)
        found = [f for f in found if not (what == "count scan" and f == "table/smt_kernels.hip")]
        assert found == [where[what]], (what, found)
    # a fetch is a struct with a lane in it: one holds the window, one the readlane head fetch, and the
    # __shfl one is the framing library's
    structs = {f: re.findall(r"\bstruct\s+(\w+)\s*\{[^}]*\blane\b[^}]*\}[^}]*\}", text) for f, text in src.items()}
    fetches = sorted((f, s) for f, names in structs.items() for s in names if s.endswith("Fetch"))
    assert fetches == [("common/smc_device.h", "HeadFetch"), ("common/smc_device.h", "WindowFetch"),
                       ("framing/smf_device.h", "WaveFetch")], fetches
    readlane = sorted(f for f, text in src.items() if "/" in f and "__builtin_amdgcn_readlane" in text)  # (the companions)
    assert readlane == ["common/smc_device.h"], readlane
    assert len(re.findall(r"__builtin_amdgcn_readlane", src["common/smc_device.h"])) == 2
    for name in ("scan_owner", "entry_table", "slot_stream", "chunk_verdict", "stream_verdict", "walker_chunk", "walker_table",
                 "walker_stream", "scan_slots", "ChunkCallArrays"):
        found = [f for f, text in src.items() if re.search(r"\b%s\b" % name, text)]
        assert not found, (name, found)
    # the slot rules and the staging's layout compile without HIP: the host checkers build them alone
    assert not re.search(r"#\s*include\s*[<\"]hip/", src["common/smc_slots.h"])
    assert not re.search(r"#\s*include\s*[<\"]hip/", src["common/smc_staging.h"])
    mk = src["common/companion.mk"].replace("\\\n", " ")
    hdrs = re.search(r"^HDRS\s*\+=(.*)$", mk, re.M).group(1).split()
    here = {"../" + f for f in src if f.startswith("common/") and f.endswith(".h")}
    assert here <= set(hdrs), (here, hdrs)
