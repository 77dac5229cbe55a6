import json, glob, os, sys
for f in sorted(glob.glob(os.path.join(os.environ.get('OUT', 'bench_out'), 'ablate', '*.json'))):
    l = [x for x in open(f) if x.startswith('{')]
    if not l:
        print(f, 'no output'); continue
    d = json.loads(l[-1]); k = d['roofline']['kernels']
    print("%-28s %9.1f  %s" % (f.split('/')[-1], d['value'], {n: v['avg_us'] for n, v in k.items()}))
