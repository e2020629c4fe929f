"""csrc/host_options.h is the only place that knows an environment knob's or a context option's name: its table and
DESIGN.md's "Tuning knobs" / "Context options" paragraphs list the same names, no other file of csrc/ reads the environment,
and `mi355tts_set_option` takes exactly the documented options."""
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "larynx_amd" / "csrc"


def design_paragraph(start: str) -> str:
    """The lines of DESIGN.md from the one that starts with `start` up to the next paragraph heading or blank line."""
    out = []
    for line in (REPO / "DESIGN.md").read_text().splitlines():
        if out and (not line.strip() or line.startswith("Context options")):
            break
        if out or line.startswith(start):
            out.append(line)
    assert out, f"DESIGN.md has no paragraph starting with {start!r}"
    return "\n".join(out)


def table_knobs():
    """(name, read time) of every row of MI355TTS_ENV_KNOBS."""
    rows = re.findall(r'^\s*X\(\w+, "(MI355TTS_\w+)", [\w ]+, [^,]+, (PROCESS|CALL),', (CSRC / "host_options.h").read_text(), re.M)
    assert len(rows) == len({n for n, _ in rows}) > 30
    return rows


def documented_knobs():
    # `MI355TTS_FORCE_TILE[_DYNAMIC]` stands for both names; the compile-time macros have a sentence of their own
    names = set()
    for m in re.findall(r"`(MI355TTS_[A-Z0-9_\[\]]+)`", design_paragraph("Tuning knobs").split("Compile-time")[0]):
        base = re.sub(r"\[\w+\]", "", m)
        names |= {base, m.replace("[", "").replace("]", "")}
    return names


def test_knob_table_and_design_list_the_same_names():
    assert {n for n, _ in table_knobs()} == documented_knobs()


def test_call_knobs_are_the_ones_tests_and_tools_move():
    assert {n for n, when in table_knobs() if when == "CALL"} == {
        "MI355TTS_FORCE_TILE_DYNAMIC", "MI355TTS_M128_MIN_TILES", "MI355TTS_GROUP_NCU", "MI355TTS_PROMOTE_MAX_IMBALANCE",
        "MI355TTS_RB_NB4_MIN_TILES", "MI355TTS_RB_PAIR_MIN_TILES", "MI355TTS_BENCH_ABLATE"}


def test_only_the_options_header_reads_the_environment():
    readers = sorted(p.name for p in CSRC.iterdir() if p.is_file() and "getenv" in p.read_text())
    assert readers == ["host_options.h"]
    # ... and every name it reads is a row of the table: no getenv with a literal of its own
    assert re.findall(r'getenv\(\s*"', (CSRC / "host_options.h").read_text()) == []


def documented_options():
    names = re.findall(r"`([a-z0-9_]+)`", design_paragraph("Context options").split("(in the fp16 mode")[0])
    assert "mi355tts_set_option" in names
    return [n for n in names if n != "mi355tts_set_option"]


def test_option_table_and_design_list_the_same_names():
    src = (CSRC / "host_options.h").read_text()
    table = re.findall(r'^\s*\{"(\w+)", (?:&ContextOptions::\w+|nullptr), (?:&ContextOptions::\w+|nullptr)\},', src, re.M)
    assert len(table) >= 15 and sorted(table) == sorted(documented_options())


def test_set_option_takes_the_documented_options(emu_library):
    from larynx_amd import ffi
    from larynx_amd.engine import Engine

    invalid = -1  # MI355TTS_ERR_INVALID (include/mi355tts.h)
    eng = Engine(device=0, library_path=emu_library)  # a context of its own: the shared one keeps its options
    try:
        for name in documented_options():
            eng.set_option(name, 3 if name == "sync_mode" else 1)  # (sync_mode is process-wide: 3 is its default)
        for name in ("glow_coalesce", "nope"):
            with pytest.raises(ffi.Mi355ttsError) as err:
                eng.set_option(name, 1)
            assert err.value.code == invalid and f"unknown option '{name}'" in str(err.value)
        with pytest.raises(ffi.Mi355ttsError) as err:
            eng.set_option("sync_mode", 4)
        assert err.value.code == invalid and "sync_mode 4 outside [0, 3]" in str(err.value)
    finally:
        eng.close()
