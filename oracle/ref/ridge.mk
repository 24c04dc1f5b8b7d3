# oracle/ref/ridge.mk -- builds oracle/_ref/<CFG>/ref_ridge: the reference's own ridge_ice (ice_mechred) with the module closure and the
# recipe of oracle/ref/Makefile (its MODS, DEFS, FC, FFLAGS: -ffp-contract=off), compiled unmodified from the sources where they lie
# and linked with our driver oracle/ref/ref_ridge.F90.  Nothing is copied into this repository; every output goes to oracle/_ref/,
# which is git-ignored.  Test infrastructure: it produces the fixtures tests/golden/ref_ridge_*.npz (tests/golden/make_ref_ridge.py).
#   make -f ridge.mk CFG=name NX=.. NY=.. BX=.. BY=.. MXB=.. NCAT=..
include Makefile

ridge: $(OUT)/ref_ridge
.DEFAULT_GOAL := ridge

$(OUT)/ref_ridge: ref_ridge.F90 ridge.mk Makefile
	@test -d $(REF)/source || { echo "oracle/_ref: $(REF) is not present (it never is on the GPU box): nothing to build"; exit 1; }
	@mkdir -p $(OUT)/g
	@set -e; cd $(OUT)/g; trap 'cd ..; rm -rf g' EXIT; objs=""; \
	for m in $(MODS); do b=$$(basename $$m); \
	  cpp -P -traditional $(DEFS) $(REF)/$$m.F90 > $$b.f90; \
	  $(FC) $(FFLAGS) -w -c $$b.f90 -o $$b.o; objs="$$objs $$b.o"; done; \
	$(FC) $(FFLAGS) -w -I. -c $(CURDIR)/ref_ridge.F90 -o ref_ridge.o; \
	$(FC) -o ../ref_ridge ref_ridge.o $$objs
	@echo "built $(OUT)/ref_ridge"
