"""CPU: the host functions of wbc_layout.h that describe the default step's instances and the packed
cycle blocks, compiled for the host from the engine's own header:

* step_args_refused(STF, SONLY, RP, CN, args): what the launcher of the instance
  wbc_update_solve_kernel<STF, SONLY, RP, CN> refuses.  Checked against a truth table of the nine
  hand-written launchers this function replaced, one row per kernel unit.
* step_instance(cn, rp, all_stance, stateful): the instance a default step takes, against the
  engine's earlier if / else-if chain.
* input_view / output_view / input_block_bytes / input_block_words / output_block_bytes: the
  packed blocks [pose | nu | qj | ref | contacts | switching] and [tau | grf | status | iters | x],
  against the sizes and offsets the engine computed by hand."""
import itertools

import pytest

from unit_reports import build_host_program, run_host_program

PROG = r"""
#include <cstdio>
#include <cstring>
#include "wbc_layout.h"
int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "names")) {
#define X(unit) std::printf("%d " #unit "\n", (int)wbc::STEP_##unit);
        WBC_STEP_UNITS(X)
#undef X
        std::printf("%d count\n", (int)wbc::STEP_INSTANCES);
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "instance")) {
        for (int i = 0; i < 16; ++i)
            std::printf("%d %d %d %d %d\n", i >> 3 & 1, i >> 2 & 1, i >> 1 & 1, i & 1,
                        (int)wbc::step_instance(i >> 3 & 1, i >> 2 & 1, i >> 1 & 1, i & 1));
        return 0;
    }
    if (argc > 1 && !std::strcmp(argv[1], "blocks")) {
        long B;
        while (std::scanf("%ld", &B) == 1) {
            // a base that is 8-byte aligned and no more, so the alignments below are the layout's own
            alignas(16) static unsigned char mem[1 << 20];
            unsigned char* base = mem + 8;
            const wbc::InputView in = wbc::input_view(static_cast<void*>(base), (size_t)B);
            const wbc::ConstInputView cin = wbc::input_view(static_cast<const void*>(base), (size_t)B);
            const wbc::ConstInputView cv = wbc::const_view(in);
            const wbc::OutputView out = wbc::output_view(base, (size_t)B);
            const bool same = cin.pose == in.pose && cin.nu == in.nu && cin.qj == in.qj && cin.ref == in.ref &&
                              cin.contacts == in.contacts && cin.switching == in.switching && cv.pose == in.pose &&
                              cv.nu == in.nu && cv.qj == in.qj && cv.ref == in.ref && cv.contacts == in.contacts &&
                              cv.switching == in.switching;
            auto off = [&](const void* p) { return (long)(static_cast<const unsigned char*>(p) - base); };
            std::printf("%ld %d %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %zu %zu %zu %zu\n", B, (int)same, off(in.pose),
                        off(in.nu), off(in.qj), off(in.ref), off(in.contacts), off(in.switching), off(out.tau), off(out.grf),
                        off(out.status), off(out.iters), off(out.x), wbc::input_block_bytes((size_t)B),
                        wbc::input_block_words((size_t)B), wbc::output_block_bytes((size_t)B),
                        wbc::output_block_bytes((size_t)B, false));
        }
        return 0;
    }
    // "refused": lines of STF SONLY RP CN nwaves stateful modes qmap rp cn (pointers: 0 = null)
    int stf, sonly, rp, cn, nwaves, stateful, modes, qmap, prp, pcn;
    static const int32_t map[4] = {0, 0, 0, 0};
    static const double tab[12] = {0};
    while (std::scanf("%d %d %d %d %d %d %d %d %d %d", &stf, &sonly, &rp, &cn, &nwaves, &stateful, &modes, &qmap, &prp,
                      &pcn) == 10) {
        wbc::KernelArgs a;
        std::memset(&a, 0, sizeof(a));
        a.nwaves = nwaves;
        a.stateful = stateful;
        a.modes = modes;
        a.qmap = qmap ? map : nullptr;
        a.rp = prp ? tab : nullptr;
        a.cn = pcn ? tab : nullptr;
        std::printf("%d\n", (int)wbc::step_args_refused(stf, sonly != 0, rp != 0, cn != 0, a));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def layout_bin(tmp_path_factory):
    """The program above, built with the address and undefined-behaviour sanitizers when the host
    toolchain links them (a stand-alone program: nothing is preloaded), else without."""
    return build_host_program(tmp_path_factory.mktemp("dispatch"), "d", PROG)


# The nine launchers as they were written by hand, one per kernel unit: (STF, SONLY, RP, CN) and the
# condition under which each returned hipErrorInvalidValue.
HAND_WRITTEN = {
    "stance": ((0, 1, 0, 0), lambda a: a["nwaves"] <= 0 or a["stateful"] or a["modes"] or a["qmap"]),
    "step0": ((0, 0, 0, 0), lambda a: a["nwaves"] <= 0 or a["stateful"]),
    "step1": ((1, 0, 0, 0), lambda a: a["nwaves"] <= 0 or not a["stateful"]),
    "rp0": ((0, 0, 1, 0), lambda a: a["nwaves"] <= 0 or a["stateful"] or a["modes"] or not a["rp"]),
    "rps": ((0, 1, 1, 0), lambda a: a["nwaves"] <= 0 or a["stateful"] or a["modes"] or a["qmap"] or not a["rp"]),
    "rp1": ((1, 0, 1, 0), lambda a: a["nwaves"] <= 0 or not a["stateful"] or a["modes"] or not a["rp"]),
    "cn0": ((0, 0, 1, 1), lambda a: a["nwaves"] <= 0 or a["stateful"] or a["modes"] or not a["rp"] or not a["cn"]),
    "cns": ((0, 1, 1, 1),
            lambda a: a["nwaves"] <= 0 or a["stateful"] or a["modes"] or a["qmap"] or not a["rp"] or not a["cn"]),
    "cn1": ((1, 0, 1, 1), lambda a: a["nwaves"] <= 0 or not a["stateful"] or a["modes"] or not a["rp"] or not a["cn"]),
}


def five_rules(inst, a):
    """What the check must refuse for any (STF, SONLY, RP, CN), units or not."""
    stf, sonly, rp, cn = inst
    return bool(a["nwaves"] <= 0 or bool(a["stateful"]) != bool(stf) or (sonly and (a["modes"] or a["qmap"])) or
                (rp and (a["modes"] or not a["rp"])) or (cn and not a["cn"]))


# 3 x 3 x 2 x 2 x 2 x 2 = 144 argument sets: no waves (0, negative) and some, stateless / stateful
# (1 and another non-zero value), hypotheses, a map, each table
ARGS = [dict(nwaves=n, stateful=s, modes=m, qmap=q, rp=r, cn=c)
        for n, s, m, q, r, c in itertools.product((-1, 0, 3), (0, 1, 2), (0, 4), (0, 1), (0, 1), (0, 1))]


def test_argument_check_is_the_nine_hand_written_ones(layout_bin):
    insts = list(itertools.product((0, 1), repeat=4))
    assert len(insts) == 16 and len(ARGS) >= 36
    text = "".join(" ".join(str(v) for v in (*inst, a["nwaves"], a["stateful"], a["modes"], a["qmap"], a["rp"], a["cn"])) + "\n"
                   for inst in insts for a in ARGS)
    got = iter(int(l[0]) for l in run_host_program(layout_bin, "refused", text))
    units = {inst: rule for inst, rule in HAND_WRITTEN.values()}
    assert len(units) == 9
    for inst in insts:
        for a in ARGS:
            g = next(got)
            if inst in units:
                assert g == int(bool(units[inst](a))), (inst, a)
            assert g == int(five_rules(inst, a)), (inst, a)
    # each rule refuses something and something passes, for every unit
    for name, (inst, rule) in HAND_WRITTEN.items():
        assert any(rule(a) for a in ARGS) and not all(rule(a) for a in ARGS), name


def earlier_chain(cn, rp, all_stance, stateful):
    """wbc_step's launcher choice as the engine wrote it out before: cn wins over rp, all_stance picks
    the stance-only instance, otherwise stateful picks 1 or 0."""
    if cn and all_stance:
        return "cns"
    if cn:
        return "cn1" if stateful else "cn0"
    if rp and all_stance:
        return "rps"
    if rp:
        return "rp1" if stateful else "rp0"
    if all_stance:
        return "stance"
    return "step1" if stateful else "step0"


def test_instance_choice_is_the_earlier_chain(layout_bin):
    names = {n: int(i) for i, n in run_host_program(layout_bin, "names")}
    assert names.pop("count") == 9 and sorted(names.values()) == list(range(9))
    assert sorted(names) == sorted(HAND_WRITTEN)
    rows = run_host_program(layout_bin, "instance")
    assert len(rows) == 16
    for cn, rp, all_stance, stateful, got in ([int(v) for v in r] for r in rows):
        if all_stance and stateful:
            # cannot occur: step_all_stance is false for a stateful step; the function need not define
            # it, it only has to name an instance
            assert 0 <= got < 9
            continue
        assert got == names[earlier_chain(cn, rp, all_stance, stateful)], (cn, rp, all_stance, stateful)


@pytest.mark.parametrize("B", [1, 3, 4, 5, 64, 65])
def test_block_views(layout_bin, B):
    (row,) = run_host_program(layout_bin, "blocks", f"{B}\n")
    v = [int(x) for x in row]
    assert v[0] == B and v[1] == 1  # the const views name the same arrays
    pose, nu, qj, ref, contacts, switching, tau, grf, status, iters, x = v[2:13]
    in_bytes, in_words, out_bytes, out_bytes_no_x = v[13:]
    # the engine's earlier in_block_bytes / out_block_bytes (WBC_POSE_LEN 7, WBC_NU_LEN 18,
    # WBC_NUM_JOINTS 12, WBC_REF_LEN 54, WBC_NV 42; doubles, then one byte each for masks and flags)
    assert in_bytes == B * (7 + 18 + 12 + 54) * 8 + 2 * B
    assert out_bytes == B * 2 * 12 * 8 + 2 * B * 4 + B * 42 * 8
    assert out_bytes_no_x == out_bytes - B * 42 * 8  # x is last: a cycle without it copies the head
    assert (pose, nu, qj, ref) == (0, 8 * 7 * B, 8 * 25 * B, 8 * 37 * B)
    assert (contacts, switching) == (8 * 91 * B, 8 * 91 * B + B) and switching + B == in_bytes
    assert (tau, grf, status, iters, x) == (0, 96 * B, 192 * B, 196 * B, 200 * B) and x + 8 * 42 * B == out_bytes
    assert status % 4 == 0 and iters % 4 == 0 and x % 8 == 0
    # whole 8-byte words for the resident copy; at B <= 4 the masks fit the one word after the doubles
    assert in_words == (in_bytes + 7) // 8 and 8 * in_words >= in_bytes > 8 * (in_words - 1)
    if B <= 4:
        assert in_words == 91 * B + 1
