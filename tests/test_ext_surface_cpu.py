"""The extension's surface, checked as plain text (nothing is built): every
source under csrc/ is compiled, every binding has a caller, and the retired
round-1 wgrad / 8p entry points stay gone.  (gemm_bt_8p3 is still bound and
tested; it joins RETIRED when gemm8p.hip goes.)"""

import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "amdtrain", "ops", "csrc")

RETIRED = ["gemm_tn", "gemm_tn_strided", "conv3x3_wgrad",
           "conv_generic_wgrad", "gemm_bt_8p", "conv3x3_8p",
           "AMDTRAIN_WGRAD2"]


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _py_files(*dirs):
    out = []
    for d in dirs:
        out += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    return sorted(out)


def _bound_names():
    names = re.findall(r'm\.def\(\s*"(\w+)"', _read(os.path.join(CSRC,
                                                                "ext.cpp")))
    assert len(names) > 30 and len(names) == len(set(names))
    return names


def test_setup_lists_exactly_the_csrc_sources():
    listed = set(re.findall(r'"(\w+\.(?:hip|cpp))"',
                            _read(os.path.join(ROOT, "setup.py"))))
    on_disk = {os.path.basename(p)
               for ext in ("*.hip", "*.cpp")
               for p in glob.glob(os.path.join(CSRC, ext))
               # hipify writes NAME_hip.hip next to NAME.hip when building
               if not p.endswith("_hip.hip")}
    assert listed == on_disk, (sorted(listed - on_disk),
                               sorted(on_disk - listed))


def test_every_binding_has_a_python_caller():
    text = "\n".join(_read(p) for p in _py_files("amdtrain", "tests"))
    unused = [n for n in _bound_names() if f".{n}(" not in text]
    assert not unused, unused


def test_retired_entry_points_stay_gone():
    """Whole identifiers: dwconv3x3_wgrad is a live kernel whose name merely
    ends in a retired one."""
    assert not set(RETIRED) & set(_bound_names())
    me = os.path.abspath(__file__)
    hits = []
    for p in _py_files("amdtrain", "tests", "tools"):
        if os.path.abspath(p) == me:
            continue
        text = _read(p)
        hits += [(os.path.relpath(p, ROOT), n) for n in RETIRED
                 if re.search(rf"(?<!\w){n}(?!\w)", text)]
    assert not hits, hits
