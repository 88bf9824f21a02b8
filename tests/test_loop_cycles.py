"""scripts/loop_cycles.py on a committed disassembly of this project's own SIR event loop
(tests/golden/sir_step_loop_gfx950.txt: the `while (alive)` loop of pf_step_kernel<kSIR, 1, kBinomial, 64> as hipcc
compiled it for gfx950, labels and instructions only)."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import loop_cycles  # noqa: E402

SNIPPET = os.path.join(REPO, "tests", "golden", "sir_step_loop_gfx950.txt")
KERNEL = "pf_step_kernelILi0ELi1ELi0ELi64E"


@pytest.mark.parametrize("mnemonic,cls", [
    ("v_mad_u64_u32", "philox_product"), ("v_bitop3_b32", "bitwise"), ("v_bfi_b32", "bitwise"), ("v_xor_b32", "bitwise"),
    ("v_mov_b32", "bitwise"), ("v_fma_f32", "arith"), ("v_fmamk_f32", "arith"), ("v_add_f64", "arith"),
    ("v_cvt_f32_f64", "arith"), ("v_pk_add_f32", "packed_f32"), ("v_cmp_nlt_f32", "compare"),
    ("v_cmp_lt_f64", "compare_f64"), ("v_cndmask_b32", "select"), ("v_rcp_f32", "transcendental"),
    ("v_log_f32", "transcendental"), ("v_rcp_f64", "transcendental_f64"), ("s_mul_hi_u32", "scalar"),
    ("s_cbranch_execz", "branch"), ("s_nop", "wait"), ("global_load_dword", "memory"),
])
def test_classes(mnemonic, cls):
    assert loop_cycles.classify(mnemonic) == cls


def _loop():
    items = loop_cycles.parse(open(SNIPPET).read())
    return loop_cycles.hot_loop(loop_cycles.kernel_slice(items, KERNEL))


def test_finds_the_event_loop_and_its_main_path():
    body = _loop()
    whole = loop_cycles.tally(body, loop_cycles.PRICES)
    main = loop_cycles.tally(loop_cycles.main_path(body), loop_cycles.PRICES)
    c = main["classes"]
    # Philox4x32-10: 15 of its 20 products on the VALU, the log and the reciprocal of one event
    assert c["philox_product"]["mnemonics"] == {"v_mad_u64_u32": 15}
    assert c["transcendental"]["mnemonics"] == {"v_log_f32": 1, "v_rcp_f32": 1}
    # the D-form loop: the channel from a sign bit, no select on the main path, the rare blocks outside it
    assert c["bitwise"]["mnemonics"].get("v_bfi_b32") == 1
    assert "select" not in c
    assert main["valu"] == 60
    assert whole["valu"] > main["valu"]
    assert any(m.startswith("v_cvt_f64_u32") for m in whole["classes"]["arith"]["mnemonics"])   # the f64 channel's block


def test_prices_are_the_tables_sums():
    body = loop_cycles.main_path(_loop())
    t = loop_cycles.tally(body, loop_cycles.PRICES)
    want = sum(r["n"] * loop_cycles.PRICES[c] for c, r in t["classes"].items() if c not in loop_cycles.UNPRICED)
    assert t["cycles"] == pytest.approx(want, abs=0.06)
    assert t["valu"] == sum(r["n"] for c, r in t["classes"].items() if c not in loop_cycles.UNPRICED)
    # a mnemonic's own price wins over its class's
    prices = dict(loop_cycles.PRICES, v_bfi_b32=4.2)
    t2 = loop_cycles.tally(body, prices)
    assert t2["cycles"] == pytest.approx(t["cycles"] + 4.2 - loop_cycles.PRICES["bitwise"], abs=0.11)


def test_command_line(tmp_path):
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert loop_cycles.main([SNIPPET, "--main-path", "--json"]) == 0
    d = json.loads(buf.getvalue())
    assert d["valu"] == 60
    prices = tmp_path / "p.json"
    prices.write_text(json.dumps({"compare": 4.3, "select": 4.2, "v_bfi_b32": 4.2}))
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert loop_cycles.main([SNIPPET, "--main-path", "--prices", str(prices)]) == 0
    last = buf.getvalue().strip().splitlines()[-1].split()
    assert last[0] == "VALU" and int(last[1]) == 60 and float(last[2]) < d["cycles"]
    with pytest.raises(SystemExit):
        loop_cycles.main([SNIPPET, "--kernel", "no_such_kernel"])
