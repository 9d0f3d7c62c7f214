"""No ROFL_* knob escapes tests/knob_matrix.py: every name of the registry has a class, every path / resource knob (every accepted value of an
enumeration) has a matrix case, no case names an unregistered variable, and the enumeration values are the ones the source accepts.
A knob added to the registry, or a value added to an `if (v == ...)` chain, fails here until it has a decision and a case.  (No GPU.)"""
import importlib.util
import os
import re

import pytest

import knob_matrix as KM

ROOT = KM.ROOT


def _registry():
    spec = importlib.util.spec_from_file_location("_gen_knob_table", os.path.join(ROOT, "scripts", "gen_knob_table.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return {name: dflt for name, dflt, _ in m.knobs()}


def test_every_knob_has_exactly_one_class():
    reg, cls = _registry(), KM.classification()
    assert sorted(cls) == sorted(reg), (sorted(set(reg) - set(cls)), sorted(set(cls) - set(reg)))
    assert all(reason.strip() for reason in KM.INERT.values())


def test_path_and_resource_knobs_have_a_case_at_a_non_default_value():
    reg, cov = _registry(), KM.covered_values()
    for k, c in KM.classification().items():
        if c in ("path", "resource"):
            assert {v for v in cov.get(k, ()) if v != reg[k]}, "%s (%s) is in no matrix case at a non-default value" % (k, c)
    # ... and among the knobs that some case's witnesses speak for, unless it is listed, with a reason, as one no witness can reach
    proved = {k for case in KM.CASES for k in case["proves"]}
    for k, c in KM.classification().items():
        if c in ("path", "resource"):
            assert (k in proved) != (k in KM.UNWITNESSED), "%s: proved by a case's witnesses XOR listed in UNWITNESSED" % k
    assert all(r.strip() for r in KM.UNWITNESSED.values()) and not set(KM.UNWITNESSED) - set(KM.classification())
    for k, (_, values) in KM.ENUMS.items():
        missing = [v for v in values if str(v) not in cov.get(k, ())]
        assert not missing, "%s: no matrix case for %s" % (k, missing)
    assert "4" in cov["ROFL_MSM_SMALL_GROUP"]      # the default of the grouped launch is a case too: only range_many reaches it


def test_cases_name_registered_knobs_and_known_workloads_only():
    reg = _registry()
    ids = KM.cases_by_id()
    for c in ids.values():
        assert re.fullmatch(r"[a-z0-9-]+", c["id"])
        assert not set(c["env"]) - set(reg), (c["id"], sorted(set(c["env"]) - set(reg)))
        assert c["workloads"] and not set(c["workloads"]) - set(KM.WORKLOADS), c["id"]
        assert c["skip_unless"] in (None, "horner8", "merlin8"), c["id"]
        if c["skip_unless"]:       # the only cases that may skip: the host-SIMD ones
            assert set(c["env"]) & {"ROFL_MSM_HOST8", "ROFL_MSM_HOST8_MIN", "ROFL_MSM_FB_HOST8_MIN", "ROFL_MERLIN_X8", "ROFL_KECCAK_ZMM"}, c["id"]
        if any(KM.classification()[k] == "path" for k in c["env"]):
            assert c["witnesses"], "%s has no witness" % c["id"]
        for w in c["witnesses"]:
            assert w[0] in ("some", "none", "count") and len(w) in (3, 4), (c["id"], w)


@pytest.mark.parametrize("knob", sorted(KM.ENUMS))
def test_enumeration_values_are_the_ones_the_source_accepts(knob):
    reg = _registry()
    dflt = KM.ENUM_DEFAULTS.get(knob, 0)
    assert str(dflt) == reg[knob]
    accepted = KM.accepted_in_source(knob)
    if knob == "ROFL_MSM_SMALL_GROUP":      # a clamp to [1, 4] in which 3 runs as 2 (the line below the read)
        src = open(os.path.join(KM.CSRC, KM.ENUMS[knob][0])).read()
        assert "J.small_group = grp == 3 ? 2 : grp;" in src
        accepted = [v for v in accepted if v != 3]
    assert sorted(v for v in accepted if v != dflt) == sorted(KM.ENUMS[knob][1]), (knob, accepted)


def test_options_point_at_tests_that_mention_them():
    for knob, where in KM.OPTION.items():
        path, name = where.split("::")
        src = open(os.path.join(ROOT, path)).read()
        m = re.search(r"^def %s\(.*?(?=^def |\Z)" % re.escape(name), src, re.S | re.M)
        assert m, where
        assert knob[len("ROFL_"):].lower() in m.group(0), (knob, where)


def test_witness_language():
    err = "\n".join(["[rofl] msm np=1 n=2000 c=4 cap=256 fb=0 lr=0 overflow=0 kind=slots two=0", "[knob-check] create a #0", "[rofl] fold K=2 tab=1", "noise", "[knob-check] verify a", "[rofl] fold K=4 tab=0"])
    out = "WITNESS x.y 3\nRESULT msm 00\n"
    assert KM.unmet([("some", "msm", {"c": "4", "n": ">1999"}), ("none", "msm", {"c": "!=4"}), ("some", "fold", {"K": "2"}, "create a #0"), ("none", "fold", {"K": "4"}, "create a #0"),
                     ("count", "x.y", ">2"), ("count", "x.y", "3")], err, out) == []
    # != on strings: "every line that is not fixed-base ran at c = 4" holds, "no line is anything but small" does not
    assert KM.unmet([("none", "msm", {"kind": "!=fb", "c": "!=4"}), ("some", "msm", {"kind": "!=small"}), ("some", "fold", {"tab": "!=x"})], err, out) == []
    assert KM.unmet([("none", "msm", {"kind": "!=small"})], err, out) == [("none", "msm", {"kind": "!=small"})]
    for junk in ("==4", ">=4", "<fb", ">", "~x"):      # a misspelt comparison raises instead of becoming a literal that never matches
        with pytest.raises(ValueError):
            KM.unmet([("some", "msm", {"c": junk})], err, out)
    bad = [("some", "msm", {"c": "7"}), ("none", "fold", {}), ("some", "fold", {"K": "2"}, "verify a"), ("count", "x.y", "4"), ("count", "x.z", "0"), ("some", "msm", {"absent": "1"})]
    assert KM.unmet(bad, err, out) == bad
