"""CPU oracle -- TEST INFRASTRUCTURE ONLY (pinned to the reference's compiled text; see aslam_oracle.h).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this package.
"""
