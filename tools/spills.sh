#!/bin/bash
# tools/spills.sh <kernel pattern>: compile rg_mpc.hip to ISA and list the kernel's spill stores with their producers
cd $(dirname $0)/.. && python3 tools/kernel_report.py --keep-isa /tmp/rg_mpc.s >/dev/null && python3 tools/isa_scratch.py /tmp/rg_mpc.s "$1" --defs
