"""Did two runs launch the same kernels?  The launches of two `rocprofv3 --kernel-trace --output-format csv -d DIR` directories in start
order, compared as (kernel name, grid, workgroup) lists; the first difference is printed and the exit status is 1.
    python tools/ab_kernel_trace.py LABEL DIR_PARENT DIR_NEW"""
import csv, glob, sys
def load(d):
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))
    assert len(f) == 1, (d, f)
    rows = list(csv.DictReader(open(f[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"], r["Workgroup_Size_Z"]) for r in rows]
a, b = load(sys.argv[2]), load(sys.argv[3])
print(f"kernel trace {sys.argv[1]:28s} parent {len(a)} launches, new {len(b)} launches ({len(set(r[0] for r in b))} distinct kernels): "
      f"ordered (name, grid, workgroup) lists {'identical' if a == b else 'DIFFERENT'}")
if a != b:
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            print("  first difference at launch", i, x, y); break
    sys.exit(1)
