"""The library's run-time switches live in one table (csrc/switches.h, filled by csrc/switches.hip; DESIGN.md "Switches").  Text
searches only: no library is built or loaded here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "map-dit_amd", "csrc")

# The A/B levers that were taken out once nothing set them any more (DESIGN.md names each with the place its verdict is recorded).
REMOVED = ["MAPDIT_GEMM_PERSIST", "MAPDIT_KEEP", "MAPDIT_GEMM_NSPLIT", "MAPDIT_GEMM_STAGGER", "MAPDIT_GEMM_BAND768", "MAPDIT_GEMM_FE",
           "MAPDIT_GEMM_DMA", "MAPDIT_GEMM_TILE_RULE", "MAPDIT_GEMM_TILE64", "MAPDIT_SPLITK_SLOTS128", "MAPDIT_RMB_NSPLIT", "MAPDIT_ATTN72",
           "MAPDIT_ATTN72_RAW", "ATTN_PROBE", "MAPDIT_EPI_PD_AUX", "MAPDIT_RMB_WIDE"]
SOURCE_SUFFIXES = (".hip", ".h", ".py", ".sh", ".md", ".txt", ".json", ".cfg", ".toml", "Makefile")


def read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def source_files(top, skip_dirs=()):
    for d, dirs, files in os.walk(top):
        dirs[:] = [x for x in dirs if x not in ("__pycache__", "_stamps", "_ab") + tuple(skip_dirs)]
        for f in sorted(files):
            if f.endswith(SOURCE_SUFFIXES):
                yield os.path.join(d, f)


def test_one_file_reads_the_environment():
    users = [os.path.basename(p) for p in source_files(CSRC) if re.search(r"\bgetenv\b", read(p))]
    assert users == ["switches.hip"], users


def test_removed_switches_are_named_nowhere():
    me = os.path.abspath(__file__)
    files = list(source_files(CSRC)) + list(source_files(os.path.join(ROOT, "include"))) + list(source_files(os.path.join(ROOT, "tests")))
    files += list(source_files(os.path.join(ROOT, "tools"), skip_dirs=("attic",)))
    files += list(source_files(os.path.join(ROOT, "map-dit_amd"), skip_dirs=("csrc",))) + [os.path.join(ROOT, "mapdit_amd.py")]
    assert len(files) > 100
    pat = re.compile(r"\b(" + "|".join(REMOVED) + r")\b")
    found = {}
    for p in files:
        if os.path.abspath(p) == me:
            continue
        names = sorted(set(pat.findall(read(p))))
        if names:
            found[os.path.relpath(p, ROOT)] = names
    assert not found, found


def design_switches_section():
    text = read(os.path.join(ROOT, "DESIGN.md"))
    m = re.search(r"^### Switches\n(.*?)^#{2,3} ", text, flags=re.S | re.M)
    assert m, "DESIGN.md has no '### Switches' section"
    return m.group(1)


def test_registry_and_design_list_the_same_switches():
    registry = re.findall(r'getenv\("([A-Z0-9_]+)"\)', read(os.path.join(CSRC, "switches.hip")))
    assert len(registry) == len(set(registry)) >= 8, registry
    section = design_switches_section()
    listed = re.findall(r"^\| `([A-Z0-9_]+)` \|", section, flags=re.M)          # the table of the survivors, one row each
    assert sorted(listed) == sorted(registry), set(listed) ^ set(registry)
    # every field of the table documents its variable, and the section says where each removed lever's verdict is
    header = read(os.path.join(CSRC, "switches.h"))
    for name in registry:
        assert re.search(r"//\s*" + name + r"\b", header), f"{name}: no comment in switches.h"
    for name in REMOVED:
        assert re.search(r"`" + name + r"`", section), f"{name}: not named in DESIGN.md's Switches section"


def test_gemm_has_no_section_owned_by_one_build():
    text = read(os.path.join(CSRC, "gemm.hip"))
    assert not re.search(r"#\s*if.*MAPDIT_DT\s*==\s*0", text)
    makefile = read(os.path.join(CSRC, "Makefile"))
    srcs = re.search(r"^SRCS\s*=(.*)$", makefile, flags=re.M).group(1).split()
    dt_srcs = re.search(r"^DT_SRCS\s*=(.*)$", makefile, flags=re.M).group(1).split()
    assert "switches.hip" in srcs and "switches.hip" not in dt_srcs
