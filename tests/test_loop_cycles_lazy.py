"""scripts/loop_cycles.py on the committed disassembly of the SIR event loop with lazily formed Philox words
(tests/golden/sir_step_loop_lazy_gfx950.txt: the `while (alive)` loop of pf_step_kernel<kSIR, 1, kBinomial, 64> and its
three rare blocks, labels and instructions only), set against the loop before it (sir_step_loop_gfx950.txt): three VALU
instructions fewer on the main path, and the last round's XORs of x, ~x and z only inside guarded blocks."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import loop_cycles  # noqa: E402

BEFORE = os.path.join(REPO, "tests", "golden", "sir_step_loop_gfx950.txt")
AFTER = os.path.join(REPO, "tests", "golden", "sir_step_loop_lazy_gfx950.txt")
KERNEL = "pf_step_kernelILi0ELi1ELi0ELi64E"


def _main(path):
    items = loop_cycles.parse(open(path).read())
    body = loop_cycles.hot_loop(loop_cycles.kernel_slice(items, KERNEL))
    return loop_cycles.tally(loop_cycles.main_path(body), loop_cycles.PRICES), loop_cycles.tally(body, loop_cycles.PRICES)


def test_main_path_lost_three_instructions():
    before, _ = _main(BEFORE)
    after, whole = _main(AFTER)
    assert before["valu"] == 60 and after["valu"] == 57
    b, a = before["classes"], after["classes"]
    # the two XORs of the last round (x / ~x and z) left the main path ...
    assert b["bitwise"]["mnemonics"]["v_bitop3_b32"] == 14 and a["bitwise"]["mnemonics"]["v_bitop3_b32"] == 12
    # ... and the compiler joined the R += ri and I += s adds into one packed add: 17 arith -> 15 + 1 packed
    assert b["arith"]["n"] == 17 and a["arith"]["n"] + a["packed_f32"]["n"] == 16
    # the stream is untouched: 15 products on the vector unit, one log and one reciprocal per event
    assert a["philox_product"]["mnemonics"] == {"v_mad_u64_u32": 15}
    assert a["transcendental"]["mnemonics"] == {"v_log_f32": 1, "v_rcp_f32": 1}
    assert after["cycles"] < before["cycles"] - 3 * loop_cycles.PRICES["bitwise"] + 0.06
    assert whole["valu"] > after["valu"]


def test_lazy_words_sit_in_guarded_blocks_only():
    items = loop_cycles.kernel_slice(loop_cycles.parse(open(AFTER).read()), KERNEL)
    # the main path: the loop up to its backward branch (the two small-x log blocks follow it and are entered from it
    # under a lane mask) without the block it guards itself (the f64 channel)
    kept = loop_cycles.main_path(loop_cycles.hot_loop(items))
    main_ops = [ops for _, m, ops in kept if m == "v_bitop3_b32"]
    rare_ops = [ops for _, m, ops in items if m == "v_bitop3_b32"]
    for ops in main_ops:
        rare_ops.remove(ops)
    assert len(main_ops) == 12 and all("bitop3:0x96" in o for o in main_ops)
    # ~x (truth table 0x69) in the 2^-20 <= 1 - U < 2^-8 block; x in the tiny_log2 block; z in the f64 channel's block
    assert sorted(o.split("bitop3:")[1] for o in rare_ops) == ["0x69", "0x96", "0x96"]
