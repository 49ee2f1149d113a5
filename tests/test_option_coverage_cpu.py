"""Every tuning option of csrc/flood_options.def is set to a non-default value by some GPU test: the tables of
``variant_cases`` (``SET_BY``: what the variant modules set; ``COVERED_ELSEWHERE``: the earlier test that sets it) must
account for every row of the option file, name a test file that exists and mentions the option, and list only values
the option accepts (the ranges of ``test_options_cpu.TABLE``).  No GPU."""
import os
import re

import test_options_cpu as oc
import variant_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")


def _option_names():
    text = open(os.path.join(ROOT, "flooder_amd", "csrc", "flood_options.def")).read()
    return re.findall(r"^FLOODER_OPTION(?:_LIST)?\(\s*(\w+)", text, re.M)


def test_every_option_is_set_by_a_gpu_test():
    names = _option_names()
    assert len(names) > 60 and len(set(names)) == len(names)
    listed = set(vc.option_values()) | set(vc.COVERED_ELSEWHERE)
    assert not set(names) - listed, f"options no GPU test sets: {sorted(set(names) - listed)}"
    assert not listed - set(names), f"listed, but no option: {sorted(listed - set(names))}"


def test_listed_values_are_accepted_and_not_the_default():
    for name, values in vc.option_values().items():
        default, accepted = oc.TABLE[name]
        assert values, name
        for v in values:
            assert v != default, (name, v)
            if isinstance(accepted, list):
                assert v in accepted, (name, v)
            else:
                assert accepted[0] <= v <= accepted[1], (name, v)


def test_the_modules_named_exist_and_set_the_option():
    for module, rows in vc.SET_BY.items():
        text = open(os.path.join(TESTS, module + ".py")).read()
        assert "pytest.mark.gpu" in text and "variant_cases" in text, module
        for name in rows:
            assert re.search(rf"\b{name}\b", text) or f'SET_BY["{module}"]' in text, (module, name)
    for name, where in vc.COVERED_ELSEWHERE.items():
        text = open(os.path.join(TESTS, where.split("::")[0])).read()
        assert "pytest.mark.gpu" in text and re.search(rf"\b{name}\b", text), (name, where)
        if "::" in where:
            assert f"def {where.split('::')[1]}(" in text, where
