"""Per-kernel totals of a rocprofv3 --pmc run (counter_collection.csv): python tools/rdf_pmc_summary.py FILE"""
import collections
import csv
import sys

tot = collections.defaultdict(lambda: collections.defaultdict(float))
calls = collections.defaultdict(set)
for row in csv.DictReader(open(sys.argv[1])):
    k = row["Kernel_Name"].split("(")[0]
    tot[k][row["Counter_Name"]] += float(row["Counter_Value"])
    calls[k].add(row["Dispatch_Id"])
for k in sorted(tot):
    if "rdf" in k or "plan" in k:
        print(k, "dispatches", len(calls[k]), " ".join("%s=%.4g" % (c, v / len(calls[k])) for c, v in sorted(tot[k].items())))
