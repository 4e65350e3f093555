"""CPU-only source check: no namespace-scope function prototype in any .hip or .cpp of plonky_amd/csrc."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a function declared but not defined at namespace scope (column 0: the sources indent nothing inside a namespace); `static`
# forward declarations of one file are fine, explicit instantiations (`template int f<C>(...)`) are no prototypes
PROTOTYPE = re.compile(
    r'^(?:template\s*<[^;{}()]*>\s*)?(?!static\b|return\b|using\b|typedef\b|template\b|namespace\b|friend\b|#)'
    r'(?:extern\s+"C"\s+)?[A-Za-z_][\w:<>\*&\s,]*?[\s\*&](\w+)\s*\((?:[^;{}()]|\([^()]*\))*\)\s*(?:const\s*)?;', re.M)


def test_no_prototypes_outside_the_headers():
    """Every function one translation unit defines and another calls is declared once, in a header the defining unit includes too
    (common.h, msm_dev.cuh, host_lane.h, host_only.h): a hand-written prototype in a .hip or .cpp is not compared with anything."""
    assert PROTOTYPE.search("int f(int a,\n      void* p = nullptr);") and PROTOTYPE.search("template <class C> int g();")
    assert not PROTOTYPE.search("static int f(int a);\nint g(int a) {\n    return f(a);\n}\ntemplate int h<C>(int);")
    csrc = os.path.join(ROOT, "plonky_amd", "csrc")
    found = []
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith((".hip", ".cpp")):
            text = open(os.path.join(csrc, fn)).read()
            text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", "", m.group()), text, flags=re.S)
            text = re.sub(r"//[^\n]*", "", text)
            found += ["%s: %s" % (fn, m.group(1)) for m in PROTOTYPE.finditer(text)]
    assert not found, found
