# Is the device code of two revisions the same, kernel by kernel?  (host-side, no GPU): bash scripts/isa_diff.sh REV_A REV_B
# Checks both revisions out as git worktrees under a temp dir, compiles each kernel unit (csrc/rtw_kernel.hip with the
# Makefile's HIPFLAGS, csrc/rtw_kernel_mesh.hip with HIPFLAGS_MESH) to device assembly, cuts the assembly at the kernel
# symbols and pairs the kernels by mangled name, so their order in the code object does not matter.  A kernel's text
# runs from its "Begin function" line to the next one: the instruction stream, the .amdhsa_kernel block and the
# resource comments.  Normalised before the comparison, and nothing else: the per-compilation __hip_cuid_<hash> symbol
# and the per-unit function index in local labels (.LBB<fn>_<n> and the loop comments' BB<fn>_<n>, .Lfunc_end<fn>,
# .Ltmp<n>), with the padding in front of a comment, which moves with a label's length.
# Compares the kernels both revisions have and lists those only one of them has ("only in REV") separately: a revision
# that adds or retires kernels is still compared on the rest.
# Prints "identical N/N" per unit, or every kernel that differs with what differs in it: "order only" when its resource
# comment lines (NumVgprs, NumSgprs, ScratchSize, Occupancy, LDSByteSize, codeLenInByte) and its count of every
# instruction mnemonic are the same, so that only the order of instructions or comments moved; else the resource lines
# and mnemonic counts that changed, and the head of the first such kernel's diff.  Exit status 1 if any kernel both
# revisions have differs.
set -e
[ $# -eq 2 ] || { echo "usage: $0 REV_A REV_B" >&2; exit 2; }
ROOT="$(git -C "$(dirname "$0")" rev-parse --show-toplevel)"
TMP="$(mktemp -d)"
trap 'git -C "$ROOT" worktree remove --force "$TMP/a" 2>/dev/null; git -C "$ROOT" worktree remove --force "$TMP/b" 2>/dev/null; rm -rf "$TMP"' EXIT
for side in a b; do
  rev="$1"; [ $side = b ] && rev="$2"
  git -C "$ROOT" worktree add --detach "$TMP/$side" "$rev" >/dev/null 2>&1
  pkg="$TMP/$side/raytracer-weekend_amd"
  hipcc="$(make -s -C "$pkg" --eval 'p-%: ; @echo $($*)' p-HIPCC)"
  main="$(make -s -C "$pkg" --eval 'p-%: ; @echo $($*)' p-HIPFLAGS)"
  mesh="$(make -s -C "$pkg" --eval 'p-%: ; @echo $($*)' p-HIPFLAGS_MESH)"
  (cd "$pkg" && $hipcc $main --offload-device-only -S csrc/rtw_kernel.hip -o "$TMP/$side.main.s") &
  (cd "$pkg" && $hipcc $mesh --offload-device-only -S csrc/rtw_kernel_mesh.hip -o "$TMP/$side.mesh.s") &
done
wait
python3 - "$TMP" "$1" "$2" <<'PY'
import collections, difflib, re, sys
tmp, rev_a, rev_b = sys.argv[1:4]

def kernels(path):
    txt = open(path).read()
    txt = txt[:txt.index('\t.section\t.AMDGPU.gpr_maximums')]
    out = {}
    parts = re.split(r'^(?=\t\.protected\t\S+ +; -- Begin function )', txt, flags=re.M)
    for p in parts[1:]:
        name = p.split()[1]
        p = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_', p)
        p = re.sub(r'\.(Lfunc_begin|Lfunc_end)\d+', r'.\1', p)
        p = re.sub(r'(?<![0-9A-Za-z_])(\.L)?BB\d+_(?=\d)', r'\1BB_', p)  # labels, and the loop comments that cite them
        p = re.sub(r'[ \t]+;', ' ;', p)  # (a longer label shifts the comment column)
        tmps = {}
        p = re.sub(r'\.Ltmp\d+', lambda m: tmps.setdefault(m.group(0), '.Ltmp#%d' % len(tmps)), p)
        # not the kernel's: the section directive of whichever function follows it, and the unit's one end-of-code
        # padding (.p2alignl / .fill), which lands behind whichever kernel comes last in .text
        out[name] = [l for l in p.splitlines()
                     if not l.startswith(('\t.section\t.text', '\t.text', '\t.p2alignl ', '\t.fill '))]
    return out

# a kernel's resource comment lines by name, and how often each instruction mnemonic occurs in it
RES = re.compile(r'; (NumVgprs|NumSgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte)\b')
def profile(lines):
    res = {m.group(1): l[2:] for l in lines for m in [RES.match(l)] if m}
    return res, collections.Counter(l.split()[0] for l in lines if l[:1] == '\t' and l[1:2] not in ('', '.', ';'))

bad = 0
for unit in ('main', 'mesh'):
    a, b = kernels(f'{tmp}/a.{unit}.s'), kernels(f'{tmp}/b.{unit}.s')
    for n in sorted(set(a) ^ set(b)):
        print(f'{unit} unit: {n} only in {rev_a if n in a else rev_b}')
    shared = [n for n in a if n in b]
    n_kern = sum(1 for n in shared if any(l.startswith('\t.amdhsa_kernel ') for l in a[n]))
    diff = next((n for n in shared if a[n] != b[n]), None)
    if diff is None:
        print(f'{unit} unit: identical {len(shared)}/{len(shared)} ({n_kern} kernels, '
              f'{sum(len(a[n]) for n in shared)} lines)')
        continue
    bad = 1
    differ = [n for n in shared if a[n] != b[n]]
    print(f'{unit} unit: identical {len(shared) - len(differ)}/{len(shared)}; {len(differ)} differ:')
    first = None
    for n in differ:
        (ra, oa), (rb, ob) = profile(a[n]), profile(b[n])
        what = [f'{ra.get(k, k)} -> {rb.get(k, k)}' for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)]
        what += [f'{m} {oa[m]} -> {ob[m]}' for m in sorted(set(oa) | set(ob)) if oa[m] != ob[m]]
        print(f'  {n}: ' + ('; '.join(what) if what else 'order only'))
        first = first or (n if what else None)
    if first:
        print(f'first changed kernel: {first}')
        print('\n'.join(list(difflib.unified_diff(a[first], b[first], rev_a, rev_b, lineterm='', n=1))[:40]))
sys.exit(bad)
PY
