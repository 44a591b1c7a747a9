# tests/cpp/test_extract_plan: the extraction's host-side kernel choice
# (form_amd/csrc/extract_plan.hpp, no HIP headers), plain g++ -Werror like its neighbours.
# Built by __graft_entry__.build():  make -C tests/cpp -f extract_plan.mk
CXX ?= g++
ROOT := ../..
CXXFLAGS ?= -O2 -std=c++17 -Wall -Wextra -Werror
all: test_extract_plan
test_extract_plan: test_extract_plan.cpp $(ROOT)/form_amd/csrc/extract_plan.hpp
	$(CXX) $(CXXFLAGS) -I$(ROOT)/form_amd/csrc -o $@ test_extract_plan.cpp
clean:
	rm -f test_extract_plan
.PHONY: all clean
