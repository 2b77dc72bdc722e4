"""The CPU-made inputs of the cases of tests/test_attention_ip_bits_gpu.py are the ones its output digests were taken on: a change of
tests/ip_adapter_common.py, tests/ip_masks_common.py or the generator behind them shows here, not as a kernel that lost its bits."""
from tests import attention_ip_bits_common as bc


def test_case_list_matches_the_fixture():
    golden = bc.load_golden()
    names = [c[0] for c in bc.cases()]
    assert sorted(golden) == sorted(names) and len(names) >= 240
    assert sum(n.startswith("masked path=1") for n in names) == 28 and sum(n.startswith("masked path=0") for n in names) == 49


def test_inputs_are_the_ones_the_digests_were_taken_on():
    golden = bc.load_golden()
    seen = {}
    for name, kind, _, params in bc.cases():
        if (kind, params) not in seen:                                  # (both paths of a case share their inputs)
            seen[(kind, params)] = bc.digest(*bc.cpu_inputs(kind, params))
        assert seen[(kind, params)] == golden[name]["inputs"], name
