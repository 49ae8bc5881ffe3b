"""tests/_plan_cases.py is what tests/test_infer_f32_plans_gpu.py runs: its batch sizes follow from the two committed launch files
by the stated rule, they cover every list and every (record, id, split-K) a plan of 1..MAX_PLAN_BATCH frames can be asked to run,
and the pool's two CPU references (float64 oracle, torch float32) agree as closely as float32 allows.  No GPU."""
import ctypes as C

import numpy as np
import torch

import _plan_cases as pc


def test_sizes_are_what_the_rule_gives_for_the_committed_files():
    d = pc.plan_doc()
    cap = pc.max_plan_batch()
    assert cap == 512 and d["table"] == [1, 8, 16, 32, 64, 128, 256] and sorted(d["plans"]) == [1, 2, 3, 4, 5, 6, 7] + d["table"][1:]
    assert pc.sizes() == list(range(1, 9)) + [9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 600]
    # the rule, restated without the helper's code: table sizes, own lists, both ends of every range of borrowers, the cap
    # with its lower neighbour, one chunked size
    want = set(d["table"]) | set(d["plans"]) | {cap - 1, cap, cap + 88}
    src = {n: pc.source(n) for n in range(1, cap + 1)}
    for n in range(1, cap + 1):
        if src[n][0] == "list" and (src.get(n - 1) != src[n] or src.get(n + 1) != src[n]):
            want.add(n)
    assert pc.sizes() == sorted(want)
    assert pc.chunks(600) == [512, 88] and pc.chunks(512) == [512] and pc.chunks(1) == [1]
    assert pc.source_id(600) == "list256+list128" and pc.source_id(37) == "list64" and pc.source_id(64) == "table64"
    assert sorted(n for ns in pc.by_source().values() for n in ns) == pc.sizes()


def test_every_list_is_borrowed_by_two_sizes_of_the_set_or_by_its_only_size():
    d = pc.plan_doc()
    cap = pc.max_plan_batch()
    run = [n for n in pc.sizes() if n <= cap]
    borrowed = 0
    for M in d["plans"]:
        who = pc.borrowers(M)
        if not who:
            assert M in d["table"], M             # a table size's list is never applied: the table resolves that plan
            continue
        borrowed += 1
        have = [n for n in run if n in who]
        assert len(have) >= min(2, len(who)), (M, who[:3], have)
        assert min(who) in have and max(who) in have
    assert borrowed == 11                         # 2..7 and 16, 32, 64, 128, 256
    for n in d["table"]:                          # and every table size runs as itself
        assert n in run and pc.source(n) == ("table", n)


def test_tune_keys_of_the_host_walk_are_held_by_the_table_and_agree_with_the_committed_lists():
    """the launch order and the tune keys derived from the module tree name exactly the records of plan_configs.json, the table
    holds an applicable entry for every one of them at every table size, and the lists plan_configs.json keeps for the table
    sizes ("as the table resolves them") are those entries"""
    from wav2lip_amd import _lib
    lib = _lib.load()
    nk = lib.w2l_tune_key_ints()
    d = pc.plan_doc()
    names = [name for name, _, _, _ in pc.launches()]
    assert len(names) == len(set(names)) == 50
    for lst in d["plans"].values():
        assert [e[0] for e in lst] == names
    tab = pc.table_entries()
    for n in d["table"]:
        keys = pc.tune_keys(n)
        assert all(len(k) == nk and k in tab for _, k in keys), n
        for (_, k), (_, cid, ks) in zip(keys, pc.expected_plan(n)):
            assert lib.w2l_tune_entry_applicable((C.c_int * nk)(*k), cid) == 1 and ks >= 1, (n, k, cid)
        assert pc.expected_plan(n) == [(a, int(b), int(c)) for a, b, c in d["plans"][n]], n


def test_every_borrowed_list_entry_is_applicable_at_both_ends_of_its_range():
    """a borrowed list was tuned at another batch size: every id it names must still be one the launch's shape accepts at the N
    that borrows it (w2l_tune_entry_applicable, the launcher's own rule), else the launch silently falls back to the heuristic"""
    from wav2lip_amd import _lib
    lib = _lib.load()
    nk = lib.w2l_tune_key_ints()
    declined = []
    for n in pc.sizes():
        for m in set(pc.chunks(n)):
            for (name, key), (_, cid, ks) in zip(pc.tune_keys(m), pc.expected_plan(m)):
                if lib.w2l_tune_entry_applicable((C.c_int * nk)(*key), cid) != 1:
                    declined.append((m, name, cid, ks))
    assert not declined, declined


def test_every_launch_a_plan_can_be_asked_to_run_is_expected_at_some_size():
    want = pc.all_expected_launches()
    have = set()
    for n in pc.sizes():
        for m in pc.chunks(n):
            have |= set(pc.expected_plan(m))
    assert len(want) >= 150 and want <= have, sorted(want - have)[:10]
    from wav2lip_amd import _lib
    lib = _lib.load()
    fams = {_lib.FAMILY_NAMES[lib.w2l_conv_config_family(c)] for _, c, _ in have}
    print("families the sizes reach: %s; %d (record, id, split-K) launches, %d ids" % (sorted(fams), len(have), len({c for _, c, _ in have})))
    assert {"wino4", "tp2s", "k3s", "split", "stem7s"} <= fams
    assert any(k > 1 for _, _, k in have)


def test_pool_references_are_finite_and_inside_the_unit_interval():
    p = pc.pool()
    assert p["ref64"].shape == p["ref32"].shape == (32, 3, 96, 96)
    for ref in (p["ref64"], p["ref32"]):
        assert bool(torch.isfinite(ref).all()) and float(ref.min()) > 0.0 and float(ref.max()) < 1.0
    print("d32 = %.3e (torch float32 forward vs float64 oracle, L-inf over 32 frames)" % p["d32"])
    assert 0.0 < p["d32"] <= 2e-6              # float32 through 50 layers: a few 1e-7; an order above means a broken reference
    idx = pc.batch_index(70)
    assert idx[0] == idx[32] == idx[64] == 0 and idx[69] == 5


def test_uint8_frames_of_the_two_cpu_forwards_differ_by_truncation_edges_only():
    p = pc.pool()
    assert p["u8_64"].shape == (32, 96, 96, 3) and p["u8_64"].dtype == np.uint8
    mism, worst = pc.u8_diff(p["u8_32"], p["u8_64"])
    print("uint8 frames, float32 vs float64: %d of %d bytes differ, by at most %d" % (mism, p["u8_64"].size, worst))
    assert worst <= 1 and mism * 10000 <= p["u8_64"].size
