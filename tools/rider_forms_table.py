"""Prints the rider-form table of DESIGN.md from tests/rider_check.py (HOST_FORMS, NON_HOSTING); `--write` replaces the block between
the markers in DESIGN.md.  tests/test_rider_hosts_cpu.py fails when the two differ."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
BEGIN, END = '<!-- rider forms: begin (tools/rider_forms_table.py) -->\n', '<!-- rider forms: end -->\n'

if __name__ == '__main__':
    import rider_check
    table = rider_check.forms_markdown()
    if '--write' in sys.argv:
        path = os.path.join(ROOT, 'DESIGN.md')
        text = open(path).read()
        a, b = text.index(BEGIN) + len(BEGIN), text.index(END)
        open(path, 'w').write(text[:a] + table + text[b:])
    else:
        sys.stdout.write(table)
