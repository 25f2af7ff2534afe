"""DEV TOOL support: the source files of the quantization search (every lamejs_amd/csrc/k_quant*.h), located
relative to this script, for the isa_* tools that attribute a listing's instructions to source lines and functions."""
import re
from pathlib import Path

CSRC = Path(__file__).resolve().parent.parent / "lamejs_amd" / "csrc"
FAMILY = sorted(p.name for p in CSRC.glob("k_quant*.h"))      # k_quant.h, the stages it includes, k_quant_fast.h, k_quant_tail.h, k_quant_probe.h
# a frame of a `.loc` comment's inline chain that lies in the family: (file, line)
FRAME = re.compile(r'\b(%s):(\d+):' % "|".join(map(re.escape, FAMILY)))


def source(name):
    """The lines of a family file; source(name)[n - 1] is line n."""
    return (CSRC / name).read_text().split("\n")


def functions():
    """{file: [(first line, function name), ...]} of the LHIP_DEV functions defined in the family, in file order."""
    out = {}
    for name in FAMILY:
        out[name] = fl = []
        for i, l in enumerate(source(name), 1):
            m = re.match(r"^(?:template.*)?LHIP_DEV\s+[\w:<>\*& ]+?\s+(\w+)\s*\(", l)
            if m and not l.rstrip().endswith(";"):
                fl.append((i, m.group(1)))
    return out


def innermost(chain):
    """(file, line) of the innermost family frame of a `.loc` comment, or None."""
    m = FRAME.search(chain)
    return (m.group(1), int(m.group(2))) if m else None
