"""Compares two gfx950 listings (the .s files `make -C neutral_amd asm` leaves in build/) function by
function, instruction for instruction, with the branch labels renumbered per function.

    python profiles/window_roulette/compare_listings.py PARENT.s NEW.s

Prints how many functions both hold, how many are identical, and the names that differ."""
import re, sys, collections
def functions(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r'^(_Z\w+|\w+):\s*(;.*)?$', line)
        if name is None:
            if m and not line.startswith('.'):
                name, body = m.group(1), []
            continue
        if line.startswith('.Lfunc_end'):
            out[name] = body
            name = None
            continue
        s = line.split(';')[0].strip()
        if not s or s.startswith('.p2align') :
            continue
        body.append(s)
    return out
def normalise(body):
    labels = {}
    def lab(m):
        return labels.setdefault(m.group(0), f".L{len(labels)}")
    return [re.sub(r'\.LBB\d+_\d+', lab, s) for s in body]
a, b = functions(sys.argv[1]), functions(sys.argv[2])
same = diff = 0
differing = []
for n in a:
    if n in b:
        if normalise(a[n]) == normalise(b[n]):
            same += 1
        else:
            diff += 1; differing.append((n, len(a[n]), len(b[n])))
print("parent functions", len(a), "new functions", len(b), "common", same + diff, "identical", same, "different", diff)
print("only in parent", [n for n in a if n not in b][:10])
print("only in new", len([n for n in b if n not in a]))
for d in differing[:20]: print(d)
