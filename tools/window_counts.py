"""Dev tool: static counts of k_pcompress's bookkeeping per barrier interval,
from a device-only assembly listing (hipcc -S --cuda-device-only with the
Makefile's flags).  For each k_pcompress instance in the file: scalar loads,
integer-division sequences (v_rcp_iflag_f32) and lgkmcnt(0) waits between
consecutive s_barriers, in program order (all wave roles together).
    usage: python tools/window_counts.py file.s"""
import re
import sys

text = open(sys.argv[1]).read()
for m in re.finditer(r"^(_ZN7dietgpu11k_pcompress\w+):[^\n]*\n(.*?)^\s+s_endpgm", text, re.S | re.M):
    name, body = m.group(1), m.group(2)
    rows, cur = [], [0, 0, 0]
    for line in body.splitlines():
        op = line.split()[0] if line.split() else ""
        if op == "s_barrier":
            rows.append(cur)
            cur = [0, 0, 0]
        elif op.startswith("s_load_") or op.startswith("s_buffer_load_"):
            cur[0] += 1
        elif op == "v_rcp_iflag_f32_e32" or op == "v_rcp_iflag_f32":
            cur[1] += 1
        elif op == "s_waitcnt" and "lgkmcnt(0)" in line:
            cur[2] += 1
    rows.append(cur)
    print(name)
    for i, (ld, dv, wt) in enumerate(rows):
        print(f"  interval {i} (barrier {i - 1 if i else 'entry'} -> {i if i < len(rows) - 1 else 'end'}): "
              f"scalar loads {ld:3d}  divisions {dv:2d}  lgkmcnt(0) waits {wt:3d}")
    print(f"  total: scalar loads {sum(r[0] for r in rows)}  divisions {sum(r[1] for r in rows)}")
